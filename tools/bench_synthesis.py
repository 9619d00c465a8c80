"""Contour smoothing and shape synthesis at the benchmark shape (T = 200 frames, A = 11 articulators, N = M = 50 points, degree 3,
12 control points, lambda 1e-3) for B = 32 and B = 4 sentences.  All timings come from one run, alternating per repeat:
  hip_spline     regularize_contours on the (B, T, A, 2, N) tensor: one as_contour_spline launch; device events around `inner`
                 calls in a row, a synchronise on both sides of the window
  torch_spline   the same fits in stock torch on the same GPU, float64: chord-length parameters, a vectorised Cox-de Boor design
                 matrix, batched normal equations, torch.linalg.solve, one matmul with the evaluation matrix; timed the same way
  copy           a plain device copy that moves as many bytes as the launch must (read 2 N floats, write 2 M floats per contour)
  forward        the model's forward pass alone (ArtSpeech(45, 11), ragged lengths, the longest T)
  forward_spline synthesize_batch: forward + smoothing with lengths, what a batch costs on the device
  synthesize     the whole synthesize() of the batch without per-frame files (numerise, pad, forward, smoothing, one download,
                 target_sequence.txt + contours.npy per sentence); host clock around a call that ends on the host
  host_loop      the reference's shape of the work: one fit per contour on the host (numpy float64: design matrix, dense normal
                 equations, numpy.linalg.solve) over `--threads` threads, after one download; host clock, `--host-repeats` times
Achieved GB/s counts 8 (N + M) bytes per contour.  The smoothed contours of hip_spline and torch_spline are compared.  No time is a
pass criterion.  Writes profiles/synthesis_bench.json.
usage: python tools/bench_synthesis.py [--repeats R] [--inner K] [--threads N] [--host-repeats H] [--batches 32,4] [--out PATH]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech  # noqa: E402
from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours  # noqa: E402
from artspeech_amd.phoneme_to_articulation.synthesis import synthesize, synthesize_batch  # noqa: E402

T, A, N, M, V = 200, 11, 50, 50, 45
DEGREE, N_CTRL, LAMBDA = 3, 12, 1e-3


def spread(times):
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def window_ms(fn, inner):
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / inner


def host_ms(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def knot_vector(K, d, **kw):
    return torch.cat([torch.zeros(d, **kw), torch.linspace(0.0, 1.0, K - d + 1, **kw), torch.ones(d, **kw)])


def design_matrix(u, K, d):
    """(..., K) values of the K basis functions at u (...,) in [0, 1]: Cox-de Boor over all functions at once, 0 / 0 = 0."""
    t = knot_vector(K, d, dtype=u.dtype, device=u.device)
    span = torch.clamp((u * (K - d)).floor().long(), max=K - d - 1) + d
    b = torch.nn.functional.one_hot(span, K + d).to(u.dtype)                 # degree 0: functions 0 .. K + d - 1
    for p in range(1, d + 1):
        n = K + d - p
        i = torch.arange(n, device=u.device)
        den_a, den_b = t[i + p] - t[i], t[i + p + 1] - t[i + 1]
        wa = torch.where(den_a > 0, (u[..., None] - t[i]) / torch.where(den_a > 0, den_a, torch.ones_like(den_a)), torch.zeros_like(den_a))
        wb = torch.where(den_b > 0, (t[i + p + 1] - u[..., None]) / torch.where(den_b > 0, den_b, torch.ones_like(den_b)),
                         torch.zeros_like(den_b))
        b = wa * b[..., :n] + wb * b[..., 1:n + 1]
    return b


def torch_spline(x, d=DEGREE, K=N_CTRL, lam=LAMBDA, m=M):
    """(..., 2, N) float32 -> (..., 2, m) float32 through float64 torch on the tensor's device"""
    p = x.double().transpose(-1, -2)                                          # (..., N, 2)
    seg = (p[..., 1:, :] - p[..., :-1, :]).norm(dim=-1)
    s = torch.cat([torch.zeros_like(seg[..., :1]), seg.cumsum(-1)], dim=-1)
    u = s / s[..., -1:]
    u[..., -1] = 1.0
    B = design_matrix(u, K, d)                                                # (..., N, K)
    D = torch.zeros(K - 2, K, dtype=p.dtype, device=p.device)
    for j in range(K - 2):
        D[j, j:j + 3] = torch.tensor([1.0, -2.0, 1.0], dtype=p.dtype, device=p.device)
    G = B.transpose(-1, -2) @ B + lam * (D.T @ D)
    c = torch.linalg.solve(G, B.transpose(-1, -2) @ p)                        # (..., K, 2)
    E = design_matrix(torch.arange(m, dtype=p.dtype, device=p.device) / (m - 1), K, d)
    return (E @ c).transpose(-1, -2).float()


def numpy_design(u, K, d, t):
    span = np.minimum((u * (K - d)).astype(np.int64), K - d - 1) + d
    b = np.zeros((len(u), K + d))
    b[np.arange(len(u)), span] = 1.0
    for p in range(1, d + 1):
        n = K + d - p
        i = np.arange(n)
        den_a, den_b = t[i + p] - t[i], t[i + p + 1] - t[i + 1]
        wa = np.divide(u[:, None] - t[i], den_a, out=np.zeros((len(u), n)), where=den_a > 0)
        wb = np.divide(t[i + p + 1] - u[:, None], den_b, out=np.zeros((len(u), n)), where=den_b > 0)
        b = wa * b[:, :n] + wb * b[:, 1:n + 1]
    return b


def host_fit(contours, d=DEGREE, K=N_CTRL, lam=LAMBDA, m=M):
    """contours (n, 2, N) float32 on the host, one fit at a time"""
    t = np.concatenate([np.zeros(d), np.linspace(0.0, 1.0, K - d + 1), np.ones(d)])
    D = np.diff(np.eye(K), n=2, axis=0)
    P, E = lam * (D.T @ D), numpy_design(np.arange(m) / (m - 1.0), K, d, t)
    out = np.empty((len(contours), 2, m), np.float32)
    for k, c in enumerate(contours):
        p = c.T.astype(np.float64)
        s = np.concatenate([[0.0], np.cumsum(np.sqrt((np.diff(p, axis=0) ** 2).sum(axis=1)))])
        u = s / s[-1]
        B = numpy_design(u, K, d, t)
        out[k] = (E @ np.linalg.solve(B.T @ B + P, B.T @ p)).T
    return out


def host_loop(x, threads):
    flat = x.cpu().numpy().reshape(-1, 2, N)
    chunks = np.array_split(flat, threads * 8)
    with ThreadPoolExecutor(threads) as pool:
        return np.concatenate(list(pool.map(host_fit, chunks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--batches", default="32,4", help="comma-separated batch sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synthesis_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_synthesis needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    result = {"T": T, "A": A, "N": N, "M": M, "degree": DEGREE, "n_ctrl": N_CTRL, "lambda": LAMBDA,
              "device": torch.cuda.get_device_name(0), "cpu_threads": args.threads, "repeats": args.repeats, "inner": args.inner,
              "host_repeats": args.host_repeats, "bytes_per_contour": 8 * (N + M), "batches": {}}
    torch.manual_seed(0)
    model = ArtSpeech(V, A).to(dev).eval()
    vocabulary = {"<blank>": 0, "<unk>": 1, **{f"ph{i:02d}": i + 2 for i in range(V - 2)}}
    names = {i: t for t, i in vocabulary.items()}
    tmp = tempfile.mkdtemp(prefix="bench_synthesis_")
    try:
        for B in [int(v) for v in args.batches.split(",")]:
            g = torch.Generator().manual_seed(B)
            lengths = sorted(torch.randint(T // 3, T + 1, (B,), generator=g).tolist(), reverse=True)
            lengths[0] = T
            rows = [torch.randint(2, V, (n,), generator=g) for n in lengths]
            sentences = [(f"s{k:03d}", [names[int(i)] for i in row]) for k, row in enumerate(rows)]
            tokens = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True).to(dev)
            with torch.no_grad():   # (B, T, A, 2, N) without padded frames: what the smoothing variants see
                x = model(torch.randint(2, V, (B, T), generator=g).to(dev), [T] * B).contiguous()
            n = B * T * A
            src, dst = torch.empty(n * (N + M), device=dev), torch.empty(n * (N + M), device=dev)

            def forward():
                with torch.no_grad():
                    return model(tokens, lengths)

            variants = (("hip_spline", window_ms, lambda: regularize_contours(x, DEGREE, N_CTRL, LAMBDA, M)),
                        ("torch_spline", window_ms, lambda: torch_spline(x)),
                        ("copy", window_ms, lambda: dst.copy_(src)),
                        ("forward", window_ms, forward),
                        ("forward_spline", window_ms, lambda: synthesize_batch(model, rows, True, DEGREE, N_CTRL, LAMBDA, M)),
                        ("synthesize", host_ms, lambda: synthesize(model, sentences, vocabulary, [f"a{k:02d}" for k in range(A)], tmp,
                                                                   batch_size=B, save_frames=False)))
            values = {}
            for _ in range(2):   # warm-up of every variant at the timed shape
                values = {name: fn() for name, _, fn in variants}
            t = {name: [] for name, _, _ in variants}
            for _ in range(args.repeats):   # alternating windows of the same run
                for name, clock, fn in variants:
                    t[name].append(clock(fn, args.inner if clock is window_ms else 1))
            host_out = host_loop(x, args.threads)   # warm-up
            t["host_loop"] = [host_ms(lambda: host_loop(x, args.threads), 1) for _ in range(args.host_repeats)]
            med = {name: float(np.median(v)) for name, v in t.items()}
            entry = {f"{name}_ms": spread(v) for name, v in t.items()}
            traffic = n * 8 * (N + M)
            hip = values["hip_spline"]
            entry.update(contours=n, traffic_bytes=traffic,
                         hip_spline_GBps=traffic / med["hip_spline"] / 1e6, copy_GBps=traffic / med["copy"] / 1e6,
                         hip_spline_over_copy=med["hip_spline"] / med["copy"],
                         torch_over_hip_spline_at_median=med["torch_spline"] / med["hip_spline"],
                         host_loop_over_hip_spline_at_median=med["host_loop"] / med["hip_spline"],
                         spline_share_of_forward_spline=1.0 - med["forward"] / med["forward_spline"],
                         max_abs_diff_hip_torch=float((hip - values["torch_spline"]).abs().max()),
                         max_abs_diff_hip_host=float(np.abs(hip.cpu().numpy().reshape(-1, 2, M) - host_out).max()),
                         max_abs_coordinate=float(hip.abs().max()))
            result["batches"][f"B{B}"] = entry
            print(json.dumps({f"B{B}": entry}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
