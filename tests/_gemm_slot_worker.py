"""Worker of tests/test_gpu_gemm_plans.py::test_split_k_without_a_counter_block (a child process: the arrival-counter blocks of
gemm_f32.hip's counters_for live as long as the process that made them, at most 64 of them).  The split-K rows whose plan sums by
arrival counters run on 70 distinct streams in turn, so the last six launches of each row find no counter block and sum their
slabs with splitk_reduce_kernel instead; every result must equal the first bit for bit (the in-kernel sum is written in that
kernel's order), and the first must be fp64-close.  sk_r4 (planned with splitk_reduce4_kernel whatever the stream has) runs on the
first stream.  One line per row; exit status 1 on any mismatch."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import torch

STREAMS = 70   # counters_for serves 64


def main():
    from test_gpu_gemm_plans import ROWS, Launch, check, host, posed
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    # torch hands out streams from a pool of 32 per priority: 70 DISTINCT ones come from the runtime itself (the library's handle
    # resolves the symbol in the HIP runtime it is linked against, the one torch has loaded)
    from artspeech_amd import _lib
    create = _lib.lib().hipStreamCreate
    create.restype, create.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    torch.zeros(1, device=dev)   # the device's context exists
    streams = []
    for _ in range(STREAMS):
        h = C.c_void_p()
        assert create(C.byref(h)) == 0 and h.value
        streams.append(torch.cuda.ExternalStream(h.value, device=dev))
    assert len({s.cuda_stream for s in streams}) == STREAMS
    bad = 0
    for name, count in (("sk_counters", STREAMS), ("sk_counters_dx", STREAMS), ("sk_shift", STREAMS), ("sk_r4", 1)):
        row = ROWS[name]
        ops, ref = posed(name, dev)
        launch = Launch(row, ops, dev)
        torch.cuda.synchronize()
        results = []
        for s in streams[:count]:
            with torch.cuda.stream(s):
                results.append(launch.run())
            torch.cuda.synchronize()
        worst = check(row, ops, ref, host(results[0]), name)
        differ = [i for i, r in enumerate(results) if not all(torch.equal(r[k], results[0][k]) for k in r)]
        bad += bool(differ)
        print(f"{name}: {'ok' if not differ else 'MISMATCH on streams ' + str(differ)}: {count} streams, error / bound {worst}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
