"""The incremental PCA fit at the thesis shape (A = 10 articulators, k = 8/4/4/3/2/4/3/3/2/2, F = 100, N = 131072 synthetic frames)
at batch sizes 256 and 8: wall time per fit (device events around whole fits, warm-up first, repeats in one call, spread
reported), both phases' kernel times from the library's own HIP-event table, the time per chain step, and scikit-learn's
IncrementalPCA on the same float32 batches on the host's threads in the same call (the comparison; skipped with a note when
scikit-learn is absent).  Writes profiles/pca_fit_bench.json.
usage: python tools/bench_pca_fit.py [--frames N] [--repeats R] [--cpu-frames M] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd import _lib  # noqa: E402
from artspeech_amd.phoneme_to_articulation.principal_components.dataset import low_rank_frames  # noqa: E402
from artspeech_amd.phoneme_to_articulation.principal_components.pca import MultiArticulatorPCA  # noqa: E402

THESIS = {"tongue": 8, "lower-lip": 4, "upper-lip": 4, "soft-palate-midline": 3, "thyroid-cartilage": 2, "arytenoid-cartilage": 4,
          "epiglottis": 3, "lower-incisor": 3, "pharynx": 2, "vocal-folds": 2}


def phases(L, fit, repeats):
    """{phase: ms per fit} from the library's event table (a run of its own: the events sit between the kernels)"""
    L.as_profile_reset()
    L.as_profile_enable(1)
    for _ in range(repeats):
        fit()
    torch.cuda.synchronize()
    L.as_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    L.as_profile_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, _, ms = line.split()
        if name.startswith("pca_"):
            out[name] = float(ms) / repeats
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=16384, help="frames of the scikit-learn run at batch size 8 (scaled up linearly)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_fit_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca_fit needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    N, A, F = args.frames, len(THESIS), 100
    frames = low_rank_frames(N, A, F, 24, torch.Generator().manual_seed(0))
    order = torch.randperm(N, generator=torch.Generator().manual_seed(0))
    x, order_dev = frames.to(dev), order.to(dev)
    result = {"shape": {"frames": N, "articulators": A, "features": F, "components": [THESIS[a] for a in sorted(THESIS)]},
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "host_threads": torch.get_num_threads(), "batch": {}}
    try:
        from sklearn.decomposition import IncrementalPCA
    except ImportError:
        IncrementalPCA = None
        result["cpu_note"] = "scikit-learn is not installed: no host comparison"
    for b in (256, 8):
        pca = MultiArticulatorPCA(THESIS, b)
        fit = lambda: pca.fit(x, order_dev)   # noqa: E731
        fit()                                 # warm-up: code objects, allocator
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fit()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        steps = -(-N // b)
        entry = {"steps": steps, "fit_ms": {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))},
                 "us_per_chain_step": 1e3 * float(np.median(times)) / steps, "phase_ms": phases(L, fit, max(1, args.repeats // 2))}
        if IncrementalPCA is not None:
            n_cpu = N if b >= 64 else min(N, args.cpu_frames)
            batches = frames[order[:n_cpu]].numpy()
            t0 = time.perf_counter()
            transformers = [IncrementalPCA(n_components=THESIS[a], batch_size=b) for a in sorted(THESIS)]
            for i in range(0, n_cpu, b):
                inputs = batches[i:i + b]
                for j, t in enumerate(transformers):
                    t.partial_fit(inputs[:, j, :])
            cpu_ms = 1e3 * (time.perf_counter() - t0)
            entry["sklearn_cpu_ms"] = cpu_ms * N / n_cpu
            entry["sklearn_cpu_frames_timed"] = n_cpu
            entry["speedup_vs_sklearn_cpu"] = entry["sklearn_cpu_ms"] / entry["fit_ms"]["median"]
            got = pca.components_["tongue"].cpu().numpy()
            if n_cpu == N:
                entry["max_abs_component_difference_vs_sklearn"] = float(np.abs(got - transformers[sorted(THESIS).index("tongue")].components_).max())
        result["batch"][str(b)] = entry
        print(json.dumps({b: entry}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
