"""Exact t-SNE on the device at the thesis size of the recogniser's feature map: N = 3300 (33 grouped tokens x 100 frames) and
N = 825, D = 128 (the thesis recogniser's 2 x 64 features), perplexity 30.  All device timings come from one run:
  fit_transform   the whole TSNE(max_iter=1000).fit_transform on device features, host clock around a call that ends on the host
  sqdist, joint_p the two one-off stages, host clock, a synchronise on both sides
  hip_iteration   as_tsne_iterate, `--inner` iterations per window (two launches each, no KL pass), device events
  torch_iteration the same exact iteration (pair terms, Z, gradient, gains, momentum step) in stock torch ops on the same GPU,
                  in windows that alternate with hip_iteration's; the two are also compared after one step from one state
  kl_pass         the extra cost of an iteration that also computes the KL divergence (two more launches)
  copy            torch's copy of an (N, N) float32 matrix: as many bytes read as one iteration reads of P
and, with --sklearn, on `--threads` host threads:
  sklearn_barnes_hut  sklearn.manifold.TSNE(method="barnes_hut") as the reference runs it (its defaults), the whole fit
  sklearn_exact       not run to the end: `--exact-evals` evaluations of sklearn.manifold._t_sne._kl_divergence (the exact objective and
                      gradient, which is all an exact iteration costs on the host) on the initial embedding, their median scaled to
                      1000 iterations; _joint_probabilities is timed once and added
pairs/s counts the N (N - 1) ordered pairs of an iteration; GB/s counts the 4 N^2 bytes of P an iteration reads.  No time is a pass
criterion.  Writes profiles/tsne_bench.json.
usage: python tools/bench_tsne.py [--sizes 3300,825] [--repeats R] [--inner K] [--threads N] [--sklearn] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_recognition import tsne  # noqa: E402

D, PERPLEXITY = 128, 30.0


def spread(times):
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def window_ms(fn):
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def features(N, seed):
    """33 token clusters in D dimensions, like a recogniser's hidden features: unit noise around centres at 3 sigma"""
    g = torch.Generator().manual_seed(seed)
    centres = 3.0 * torch.randn(33, D, generator=g)
    return centres[torch.arange(N) % 33] + torch.randn(N, D, generator=g)


def torch_iterations(P, Y, update, gains, n, exaggeration, momentum, lr, min_gain=0.01):
    """n exact iterations in stock torch ops, in place on Y, update and gains"""
    for _ in range(n):
        diff = Y[:, None, :] - Y[None, :, :]
        num = 1.0 / (1.0 + (diff * diff).sum(dim=2))
        num.fill_diagonal_(0.0)
        Z = num.sum()
        w = (exaggeration * P - num / Z) * num
        grad = 4.0 * (w.sum(dim=1, keepdim=True) * Y - w @ Y)
        inc = update * grad < 0.0
        gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=min_gain))
        update.mul_(momentum).sub_(lr * gains * grad)
        Y.add_(update)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3300,825")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--exact-evals", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    result = {"D": D, "perplexity": PERPLEXITY, "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
              "repeats": args.repeats, "inner": args.inner, "sizes": {}}
    for N in [int(v) for v in args.sizes.split(",")]:
        Xh = features(N, N)
        X = Xh.to(dev)
        lr = max(N / 12.0 / 4.0, 50.0)
        for _ in range(2):   # warm-up of every stage at the timed shape
            dist = tsne.squared_distances(X)
            P = tsne.joint_probabilities(dist, PERPLEXITY)[0]
        Y0 = tsne.pca_init(X)
        state = lambda: (Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0))   # noqa: E731
        # one step from one state, both ways
        a, b = state(), state()
        tsne.iterate(P, *a, 1, 0, 12.0, 0.5, lr, kl_every=0)
        torch_iterations(P, *b, 1, 12.0, 0.5, lr)
        step_diff = float((a[0] - b[0]).abs().max() / b[0].abs().max())
        hip, tor, hip_kl = state(), state(), state()
        ws = tsne._workspace(N, dev)
        copy_dst = torch.empty_like(P)
        variants = (("hip_iteration", lambda: tsne.iterate(P, *hip, args.inner, 0, 12.0, 0.5, lr, kl_every=0, ws=ws), args.inner),
                    ("torch_iteration", lambda: torch_iterations(P, *tor, args.inner, 12.0, 0.5, lr), args.inner),
                    ("hip_iteration_with_kl", lambda: tsne.iterate(P, *hip_kl, args.inner, 0, 12.0, 0.5, lr, kl_every=1, ws=ws), args.inner),
                    ("copy", lambda: [copy_dst.copy_(P) for _ in range(args.inner)], args.inner))
        for _, fn, _ in variants:
            fn()
        t = {name: [] for name, _, _ in variants}
        for _ in range(args.repeats):   # alternating windows of the same run
            for name, fn, per in variants:
                t[name].append(window_ms(fn) * 1e3 / per)   # microseconds per iteration (per copy)
        stages = {"sqdist_ms": [], "joint_p_ms": [], "fit_transform_ms": []}
        fitted = None
        for _ in range(3):
            stages["sqdist_ms"].append(host_ms(lambda: tsne.squared_distances(X)))
            stages["joint_p_ms"].append(host_ms(lambda: tsne.joint_probabilities(dist, PERPLEXITY)))
            fitted = tsne.TSNE(perplexity=PERPLEXITY, max_iter=1000, init="pca", random_state=0)
            stages["fit_transform_ms"].append(host_ms(lambda: fitted.fit_transform(X)))
        med = {name: float(np.median(v)) for name, v in t.items()}
        entry = {f"{name}_us": spread(v) for name, v in t.items()}
        entry.update({name: spread(v) for name, v in stages.items()})
        entry.update(pairs=N * (N - 1), p_bytes=4 * N * N,
                     pairs_per_s_at_median=N * (N - 1) / (med["hip_iteration"] * 1e-6),
                     p_gb_per_s_at_median=4 * N * N / (med["hip_iteration"] * 1e-6) / 1e9,
                     copy_read_gb_per_s_at_median=4 * N * N / (med["copy"] * 1e-6) / 1e9,
                     kl_pass_us_at_median=med["hip_iteration_with_kl"] - med["hip_iteration"],
                     torch_over_hip_iteration_at_median=med["torch_iteration"] / med["hip_iteration"],
                     one_step_max_diff_over_max_y=step_diff, n_iter=fitted.n_iter_, kl_divergence=fitted.kl_divergence_,
                     launches_per_iteration=2)
        if args.sklearn:
            from sklearn.manifold import TSNE as SkTSNE
            from sklearn.manifold import _t_sne
            from sklearn.metrics import pairwise_distances
            Xn = Xh.numpy()
            t0 = time.perf_counter()
            bh = SkTSNE(n_components=2, random_state=0).fit(Xn)
            entry["sklearn_barnes_hut_ms"] = (time.perf_counter() - t0) * 1e3
            entry["sklearn_barnes_hut_n_iter"], entry["sklearn_barnes_hut_kl"] = int(bh.n_iter_), float(bh.kl_divergence_)
            t0 = time.perf_counter()
            Pc = _t_sne._joint_probabilities(pairwise_distances(Xn, metric="euclidean", squared=True), PERPLEXITY, 0)
            joint_ms = (time.perf_counter() - t0) * 1e3
            y0 = Y0.cpu().numpy().astype(np.float64).ravel()
            evals = []
            for _ in range(args.exact_evals):
                t0 = time.perf_counter()
                _t_sne._kl_divergence(y0, Pc * 12.0, 1, N, 2, compute_error=False)
                evals.append((time.perf_counter() - t0) * 1e3)
            entry.update(sklearn_joint_probabilities_ms=joint_ms, sklearn_exact_gradient_ms=spread(evals),
                         sklearn_exact_1000_iterations_ms_scaled=joint_ms + 1000 * float(np.median(evals)),
                         sklearn_exact_scaled_from=f"{args.exact_evals} evaluations of _kl_divergence on the initial embedding")
        result["sizes"][f"N{N}"] = entry
        print(json.dumps({f"N{N}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
