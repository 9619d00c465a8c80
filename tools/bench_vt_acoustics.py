"""The vocal-tract acoustics at the benchmark shape (T = 200 frames, K = 99 sections, F = 500 bins from 10 Hz in steps of 10 Hz,
five formants, three refinement rounds, the piston) for B = 32 and B = 4 sentences.  All timings come from one run, alternating per
repeat:
  hip_formants        formants() on (B T, K) sections of unequal lengths, as the area function gives them: one as_vt_acoustics
                      launch, a sine/cosine pair per (bin, section); device events around `inner` calls in a row
  hip_formants_equal  the same on sections of equal lengths, as after evenly_spaced_fx: one pair per bin
  hip_transfer        transfer_function() with the denominator: the launch without formants, with both complex128 stores
  torch_chain         the same chain product as batched complex128 stock-torch ops on the same GPU: K matrix products of
                      (B T, F, 2, 2), then den = C Z + D; no formant search; timed the same way
  host_loop           the numpy restatement (tests/vt_acoustics_fp64.py: chain, den and the formant search) over `--threads` host
                      threads; host clock
hip_formants is compared with torch_chain and with the restatement.  `den_error_over_yardstick` is the parity ratio of
tests/test_gpu_vt_acoustics.py on the first `--parity-frames` frames: max over them of (device against the longdouble
restatement) / (16 max(e64, K 2^-52)); at most 1 passes.  No time is a pass criterion.  Writes profiles/vt_acoustics_bench.json.
usage: python tools/bench_vt_acoustics.py [--repeats R] [--inner K] [--threads N] [--host-repeats H] [--batches 32,4] [--out PATH]"""
import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vt_acoustics_fp64 as R  # noqa: E402
from artspeech_amd import vocal_tract_acoustics as V  # noqa: E402
from bench_synthesis import host_ms, spread, window_ms  # noqa: E402

T, K, F, N_FORMANTS, ROUNDS, F0, DF = 200, 99, 500, 5, 3, 10.0, 10.0


def torch_chain(areas, lengths, c=R.C_SOUND, rho=R.RHO):
    """den (n, F) complex128 by stock torch ops: the 2 x 2 complex chain product section by section, then the piston."""
    n = areas.shape[0]
    f = F0 + DF * torch.arange(F, dtype=torch.float64, device=areas.device)
    k = (2 * np.pi * f / c)[None, :]
    P = torch.eye(2, dtype=torch.complex128, device=areas.device).expand(n, F, 2, 2)
    for i in range(areas.shape[1]):
        kl = k * lengths[:, i, None]
        z = (rho * c / areas[:, i])[:, None]
        cs, sn = torch.cos(kl), torch.sin(kl)
        zero = torch.zeros_like(cs)
        M = torch.stack([torch.complex(cs, zero), torch.complex(zero, z * sn), torch.complex(zero, sn / z), torch.complex(cs, zero)],
                        dim=-1).view(n, F, 2, 2)
        P = P @ M
    last = areas[:, -1, None]
    ka = 2 * np.pi * f[None, :] * torch.sqrt(last / np.pi) / c
    Z = (rho * c / last) * torch.complex(ka * ka / 2, 8 * ka / (3 * np.pi))
    return P[..., 1, 0] * Z + P[..., 1, 1]


def host_loop(areas, lengths, threads):
    chunks = np.array_split(np.arange(len(areas)), threads * 4)
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda i: R.formants(areas[i], lengths[i], f0=F0, df=DF, F=F, n_formants=N_FORMANTS, rounds=ROUNDS), chunks))
    return [np.concatenate([p[j] for p in parts]) for j in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--parity-frames", type=int, default=64)
    ap.add_argument("--batches", default="32,4", help="comma-separated batch sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vt_acoustics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vt_acoustics needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    result = {"T": T, "K": K, "F": F, "n_formants": N_FORMANTS, "rounds": ROUNDS, "f0": F0, "df": DF, "radiation": "piston",
              "device": torch.cuda.get_device_name(0), "cpu_threads": args.threads, "repeats": args.repeats, "inner": args.inner,
              "host_repeats": args.host_repeats, "parity_frames": args.parity_frames, "batches": {}}
    for B in [int(v) for v in args.batches.split(",")]:
        frames = B * T
        rng = np.random.default_rng(B)
        areas_h, lengths_h = R.draw(rng, 2 * frames, K)
        areas_h, lengths_h, equal_h = areas_h[0::2], lengths_h[0::2], lengths_h[1::2]   # R.draw: every second frame is equal-length
        areas, lengths, equal = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (areas_h, lengths_h, equal_h))
        kw = dict(f0=F0, df=DF, n_freq=F)
        variants = (("hip_formants", lambda: V.formants(areas, lengths, n_formants=N_FORMANTS, rounds=ROUNDS, **kw)),
                    ("hip_formants_equal", lambda: V.formants(areas, equal, n_formants=N_FORMANTS, rounds=ROUNDS, **kw)),
                    ("hip_transfer", lambda: V.transfer_function(areas, lengths, return_denominator=True, **kw)),
                    ("torch_chain", lambda: torch_chain(areas, lengths)))
        values = {}
        for _ in range(2):   # warm-up of every variant at the timed shape
            values = {name: fn() for name, fn in variants}
        t = {name: [] for name, _ in variants}
        for _ in range(args.repeats):   # alternating windows of the same run
            for name, fn in variants:
                t[name].append(window_ms(fn, args.inner))
        host = None
        t["host_loop"] = []
        for _ in range(args.host_repeats):
            t["host_loop"].append(host_ms(lambda: host_loop(areas_h, lengths_h, args.threads), 1))
        host = host_loop(areas_h[:args.parity_frames], lengths_h[:args.parity_frames], args.threads)
        med = {name: float(np.median(v)) for name, v in t.items()}
        entry = {f"{name}_ms": spread(v) for name, v in t.items()}
        # parity on the first frames: the device's den against the longdouble restatement, in units of the tests' yardstick
        p = args.parity_frames
        den = values["hip_transfer"][2][:p].cpu().numpy()
        d64 = R.transfer(areas_h[:p], lengths_h[:p], f0=F0, df=DF, F=F)[0]
        dl = R.transfer(areas_h[:p], lengths_h[:p], f0=F0, df=DF, F=F, dtype=np.longdouble)[0]
        scale = np.abs(dl).max(1)
        e64 = (np.abs(d64 - dl).max(1) / scale).astype(np.float64)
        err = (np.abs(den - dl).max(1) / scale).astype(np.float64)
        fm = values["hip_formants"]
        entry.update(frames=frames, torch_over_hip_formants_at_median=med["torch_chain"] / med["hip_formants"],
                     host_loop_over_hip_formants_at_median=med["host_loop"] / med["hip_formants"],
                     unequal_over_equal_lengths=med["hip_formants"] / med["hip_formants_equal"],
                     den_error_over_yardstick=float((err / (16 * np.maximum(e64, K * 2.0 ** -52))).max()),
                     den_error_max=float(err.max()), e64_max=float(e64.max()),
                     max_abs_diff_den_hip_torch=float((values["hip_transfer"][2] - values["torch_chain"]).abs().max()),
                     max_formant_diff_hip_host_hz=float(np.nanmax(np.abs(fm.frequencies[:p].cpu().numpy() - host[0]))),
                     found_equal_hip_host=bool(np.array_equal(fm.found[:p].cpu().numpy(), host[2])))
        result["batches"][f"B{B}"] = entry
        print(json.dumps({f"B{B}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
