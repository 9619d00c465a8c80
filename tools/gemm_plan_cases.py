"""Every as_gemm descriptor of tests/golden/gemm_plan_rows.json (the shapes of the GEMM tests and of the Python call sites at the
benchmark's sizes; pointers are recorded as 0 = absent or 16 + the address's low four bits) through as_gemm_f32 with seeded
operands, in both matrix arithmetics: one line per row and mode with the SHA-256 of C, colsum and relu_bits (or `refused`).
Two commits choose the same kernels when their digest files are equal and, under
`rocprofv3 --kernel-trace --output-format csv -- python tools/gemm_plan_cases.py`, their kernel sequences are.
usage: python tools/gemm_plan_cases.py [--rows FILE] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = os.path.join(ROOT, "tests", "golden", "gemm_plan_rows.json")
POINTERS = ("A", "B", "C", "bias", "splitk_ws", "colsum", "a_off", "b_off", "c_off", "bias_off", "res", "res_off", "mask_bits",
            "relu_bits", "a_seg_off", "b_seg_off")


def load_rows(path=ROWS):
    with open(path) as f:
        return json.load(f)


def up4(n):
    return (n + 3) // 4 * 4


def pose(r, dev):
    """The row's descriptor fields over freshly allocated operands, and the outputs to digest."""
    import torch
    f32 = torch.float32

    def buf(n, bits, fill=None, dtype=f32):
        t = torch.empty(n + 4, dtype=dtype, device=dev)
        if fill is None:
            t = torch.randn(n + 4, device=dev) if dtype == f32 else torch.randint(-2**31, 2**31 - 1, (n + 4,), dtype=dtype, device=dev)
        else:
            t.fill_(fill)
        return t[(bits & 15) // 4:]          # the recorded misalignment, in whole elements

    def table(n, step):
        return torch.arange(n, dtype=torch.int64, device=dev) * step

    M, N, K, batch = r["M"], r["N"], r["K"], r["batch"]
    nseg = K // r["k_seg"] if r["k_seg"] else 1
    kspan = r["k_seg"] or K
    ext_a = up4((M - 1) * r["a_i"] + (kspan - 1) * r["a_k"] + 1)
    ext_b = up4((N - 1) * r["b_j"] + (kspan - 1) * r["b_k"] + 1)
    ext_c = up4((M - 1) * r["ldc"] + N)
    ncb = (N + 31) // 32
    d, keep = {k: v for k, v in r.items() if k not in POINTERS and k != "name"}, []

    def operand(name, ext, stride, off, seg=None, **kw):
        if not r[name]:
            return None
        if seg and r["k_seg"]:
            d[seg] = table(batch * nseg, ext)
            n = batch * nseg * ext
        elif off and r[off]:
            d[off] = table(batch, ext)
            n = batch * ext
        else:
            n = (batch - 1) * max(stride, 0) + ext
        d[name] = buf(n, r[name], **kw)
        keep.append(d[name])
        return d[name]

    operand("A", ext_a, r["a_batch"], "a_off", "a_seg_off")
    operand("B", ext_b, r["b_batch"], "b_off", "b_seg_off")
    c = operand("C", ext_c, r["c_batch"], "c_off", fill=None if r["accumulate"] else float("nan"))
    operand("bias", up4(N), r["bias_batch"], "bias_off")
    operand("res", up4((M - 1) * r["res_ld"] + N), r["res_batch"], "res_off")
    cs = operand("colsum", M, r["colsum_batch"], None, fill=float("nan"))
    operand("mask_bits", M * ncb, r["mask_batch"], None, dtype=torch.int32)
    bits = operand("relu_bits", M * ncb, r["relu_bits_batch"], None, fill=-1, dtype=torch.int32)
    if r["splitk_ws"]:
        d["splitk_ws"] = torch.empty(r["splitk_ws_floats"], device=dev)
    return d, [c, cs, bits]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=ROWS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from artspeech_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    keep = L.as_get_matrix_arith()
    out = open(args.out, "w") if args.out else sys.stdout
    print(f"# compute units {torch.cuda.get_device_properties(dev).multi_processor_count}", file=out)
    for i, r in enumerate(load_rows(args.rows)):
        for mode in (0, 1):
            L.as_set_matrix_arith(mode)
            torch.manual_seed(i)
            fields, outs = pose(r, dev)
            rc = L.as_gemm_f32(_lib.C.byref(_lib.gemm_desc(**fields)), _lib.stream_ptr())
            torch.cuda.synchronize()
            if rc != 0:
                print(f"{r['name']} arith={mode} refused ({rc})", file=out, flush=True)
                continue
            sha = ["-" if t is None else hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32] for t in outs]
            print(f"{r['name']} arith={mode} C={sha[0]} colsum={sha[1]} relu_bits={sha[2]}", file=out, flush=True)
            del fields, outs
    L.as_set_matrix_arith(keep)


if __name__ == "__main__":
    main()
