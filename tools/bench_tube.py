"""The vocal-tract tube at the benchmark shape (T = 200 frames, A = 11 articulators, N = 50 points, M = 100 wall points, the default
chains of six contours) for B = 32 and B = 4 sentences.  All timings come from one run, alternating per repeat:
  hip_tube       vocal_tract_tube on the (B, T, A, 2, N) tensor: one as_vocal_tract_tube launch; device events around `inner`
                 calls in a row, a synchronise on both sides of the window
  torch_tube     the same computation in stock torch ops on the same GPU: pairwise distances -> argmin -> gather -> cumsum ->
                 searchsorted -> lerp, float32 junctions and float64 resampling as the definition has them; timed the same way
  copy           a plain device copy that moves as many bytes as the launch must (read 2 N floats per chain contour, write 2 M
                 doubles per wall)
  forward_spline synthesize_batch: the model's forward pass and the smoothing, what a batch cost on the device before the tube
  synthesize / synthesize_air_column   the whole synthesize() of the batch without per-frame contour files, without and with
                 air_column (which adds the launch, one download and the air_column/ and xarticul/ files); host clock
  host_loop      the per-frame numpy restatement (tests/tube_fp64.py) over `--threads` threads, after one download; host clock
Achieved GB/s counts the algorithmic traffic above.  hip_tube is compared with torch_tube and with the restatement.  No time is a
pass criterion: the stock-torch variant on the same GPU is the yardstick.  Writes profiles/tube_bench.json.
usage: python tools/bench_tube.py [--repeats R] [--inner K] [--threads N] [--host-repeats H] [--batches 32,4] [--out PATH]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tube_fp64 as R  # noqa: E402
from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech  # noqa: E402
from artspeech_amd.phoneme_to_articulation.synthesis import synthesize, synthesize_batch  # noqa: E402
from artspeech_amd.phoneme_to_articulation.vocal_tract_tube import EXTERNAL_WALL, INTERNAL_WALL, chain_indices, vocal_tract_tube  # noqa: E402
from bench_synthesis import host_ms, spread, window_ms  # noqa: E402

T, A, N, M, V = 200, 11, 50, 100, 45
# channel names such that R.random_frames' inner arc (even channels) is the internal wall and its outer arc the external wall
NAMES = [None] * A
NAMES[0::2] = INTERNAL_WALL
NAMES[1::2] = EXTERNAL_WALL[1:]


def torch_wall(x, chain, m=M):
    """x (F, A, 2, N) float32 on the GPU, chain: channel indices -> (F, 2, m) float64, the definition in stock torch ops"""
    F, K, n = x.shape[0], len(chain), x.shape[-1]
    pts = x[:, chain].transpose(-1, -2)                                        # (F, K, N, 2) float32
    first_e = torch.zeros(F, dtype=torch.long, device=x.device)
    entry, exit_ = torch.zeros(F, K, dtype=torch.long, device=x.device), torch.full((F, K), n - 1, dtype=torch.long, device=x.device)
    if K > 1:
        d = pts[:, :-1, :, None, :] - pts[:, 1:, None, :, :]                   # (F, K-1, N, N, 2)
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        flat = d2.flatten(2).argmin(-1)
        ji, jj = flat // n, flat % n
        exit_[:, :-1], entry[:, 1:] = ji, jj
        first_e = torch.where(ji[:, 0] >= n - 1 - ji[:, 0], 0, n - 1)
        entry[:, 0] = first_e
        last = entry[:, -1]
        exit_[:, -1] = torch.where(last <= n - 1 - last, n - 1, 0)
    length = (exit_ - entry).abs() + 1
    first = length.cumsum(-1) - length                                         # (F, K)
    P = length.sum(-1)
    p = torch.arange(K * n, device=x.device).expand(F, K * n)
    p = torch.minimum(p, (P - 1)[:, None])                                     # the points past P repeat the last one
    k = (torch.searchsorted(first, p, right=True) - 1)
    idx = entry.gather(1, k) + torch.sign(exit_ - entry).gather(1, k) * (p - first.gather(1, k))
    q = pts.flatten(1, 2).gather(1, (k * n + idx)[..., None].expand(-1, -1, 2)).double()   # (F, K N, 2)
    seg = (q[:, 1:] - q[:, :-1]).pow(2).sum(-1).sqrt()
    s = torch.cat([torch.zeros_like(seg[:, :1]), seg.cumsum(-1)], dim=-1)
    L = s[:, -1:]
    t = torch.arange(m, dtype=torch.float64, device=x.device) * L / (m - 1)
    at = torch.minimum((torch.searchsorted(s, t, right=True) - 1).clamp(min=0), (P - 2)[:, None])
    s0, s1 = s.gather(1, at), s.gather(1, at + 1)
    f = torch.where(s1 > s0, (t - s0) / torch.where(s1 > s0, s1 - s0, torch.ones_like(s0)), torch.zeros_like(s0))
    q0 = q.gather(1, at[..., None].expand(-1, -1, 2))
    q1 = q.gather(1, (at + 1)[..., None].expand(-1, -1, 2))
    out = q0 + f[..., None] * (q1 - q0)
    out[:, 0], out[:, -1] = q[:, 0], q.gather(1, (P - 1)[:, None, None].expand(-1, 1, 2))[:, 0]
    return out.transpose(-1, -2)


def torch_tube(x, chains):
    flat = x.flatten(0, -4)
    return torch.stack([torch_wall(flat, chains[0]), torch_wall(flat, chains[1])], dim=1).reshape(x.shape[:-3] + (2, 2, M))


def host_loop(x, chains, threads):
    flat = x.cpu().numpy().reshape(-1, A, 2, N)
    chunks = np.array_split(flat, threads * 8)
    with ThreadPoolExecutor(threads) as pool:
        return np.concatenate(list(pool.map(lambda c: R.tube(c, chains[0], chains[1], M)[0], chunks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--batches", default="32,4", help="comma-separated batch sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tube needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    chains = [chain_indices(NAMES, INTERNAL_WALL), chain_indices(NAMES, EXTERNAL_WALL)]
    bytes_per_frame = sum(len(c) for c in chains) * 2 * N * 4 + 2 * 2 * M * 8
    result = {"T": T, "A": A, "N": N, "M": M, "chains": [len(c) for c in chains], "device": torch.cuda.get_device_name(0),
              "cpu_threads": args.threads, "repeats": args.repeats, "inner": args.inner, "host_repeats": args.host_repeats,
              "bytes_per_frame": bytes_per_frame, "batches": {}}
    torch.manual_seed(0)
    model = ArtSpeech(V, A).to(dev).eval()
    vocabulary = {"<blank>": 0, "<unk>": 1, **{f"ph{i:02d}": i + 2 for i in range(V - 2)}}
    names = {i: t for t, i in vocabulary.items()}
    tmp = tempfile.mkdtemp(prefix="bench_tube_")
    try:
        for B in [int(v) for v in args.batches.split(",")]:
            g = torch.Generator().manual_seed(B)
            lengths = sorted(torch.randint(T // 3, T + 1, (B,), generator=g).tolist(), reverse=True)
            lengths[0] = T
            rows = [torch.randint(2, V, (n,), generator=g) for n in lengths]
            sentences = [(f"s{k:03d}", [names[int(i)] for i in row]) for k, row in enumerate(rows)]
            x = torch.from_numpy(R.random_frames(np.random.default_rng(B), B * T, A, N).reshape(B, T, A, 2, N)).to(dev)
            frames = B * T
            words = frames * bytes_per_frame // 4
            src, dst = torch.empty(words // 2, device=dev), torch.empty(words // 2, device=dev)   # a copy reads and writes each byte

            def synth(air_column):
                return synthesize(model, sentences, vocabulary, sorted(NAMES), tmp, batch_size=B, save_frames=False, air_column=air_column)

            variants = (("hip_tube", window_ms, lambda: vocal_tract_tube(x, NAMES, n_out=M)),
                        ("torch_tube", window_ms, lambda: torch_tube(x, chains)),
                        ("copy", window_ms, lambda: dst.copy_(src)),
                        ("forward_spline", window_ms, lambda: synthesize_batch(model, rows)),
                        ("synthesize", host_ms, lambda: synth(False)),
                        ("synthesize_air_column", host_ms, lambda: synth(True)))
            values = {}
            for _ in range(2):   # warm-up of every variant at the timed shape
                values = {name: fn() for name, _, fn in variants}
            t = {name: [] for name, _, _ in variants}
            for _ in range(args.repeats):   # alternating windows of the same run
                for name, clock, fn in variants:
                    t[name].append(clock(fn, args.inner if clock is window_ms else 1))
            host_out = host_loop(x, chains, args.threads)   # warm-up
            t["host_loop"] = [host_ms(lambda: host_loop(x, chains, args.threads), 1) for _ in range(args.host_repeats)]
            med = {name: float(np.median(v)) for name, v in t.items()}
            entry = {f"{name}_ms": spread(v) for name, v in t.items()}
            traffic = frames * bytes_per_frame
            hip = values["hip_tube"]
            entry.update(frames=frames, traffic_bytes=traffic, hip_tube_GBps=traffic / med["hip_tube"] / 1e6,
                         copy_GBps=traffic / med["copy"] / 1e6, hip_tube_over_copy=med["hip_tube"] / med["copy"],
                         torch_over_hip_tube_at_median=med["torch_tube"] / med["hip_tube"],
                         host_loop_over_hip_tube_at_median=med["host_loop"] / med["hip_tube"],
                         tube_over_forward_spline=med["hip_tube"] / med["forward_spline"],
                         air_column_cost_of_synthesize_ms=med["synthesize_air_column"] - med["synthesize"],
                         max_abs_diff_hip_torch=float((hip - values["torch_tube"]).abs().max()),
                         max_abs_diff_hip_host=float(np.abs(hip.cpu().numpy().reshape(-1, 2, 2, M) - host_out).max()))
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
