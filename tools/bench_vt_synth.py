"""Speech synthesis from the tube: the waveguide ladder and the glottal source on the GPU, at B = 32 and 4 utterances of T = 200
frames, S = 882 samples per frame (44.1 kHz at 50 frames per second), K = 22 sections, plus K = 44 at S = 1764 (88.2 kHz).
Variants, timed in alternating windows of the same run (HIP events around `--inner` calls, `--repeats` windows each):
  hip_ladder      waveguide(): one as_vt_waveguide launch, with frication, float32 output (the entry point reads the section
                  counts back before its launch; that wait is inside the window)
  hip_source      glottal_source(): one as_vt_glottal_source launch
  hip_end_to_end  synthesize_speech() from ragged sections: equal_sections and frication_control (torch ops), then both launches
and, outside the windows,
  torch_loop      the same recurrence as a per-sample loop of stock torch ops on the same GPU (float64, the whole batch per op,
                  no frication), timed on `--loop-samples` samples and SCALED to T S samples: `scaled_ms`
  host_loop       the numpy restatement (tests/vt_synth_fp64.py, float64) over `--threads` host threads, the utterances split
                  among them, timed on `--loop-samples` samples and SCALED likewise
Derived: seconds of audio per second of ladder launch, nanoseconds per recurrent step (launch time / samples of ONE utterance:
the utterances run side by side, one wave each), the end-to-end time beside the ladder alone.  The kernel time alone (without
the launch and the read-back) is not measured.  Parity: the device's out64 on the first `--loop-samples` samples against the
torch loop and against the restatement.  No time is a pass criterion.  Writes profiles/vt_synth_bench.json.
usage: python tools/bench_vt_synth.py [--repeats R] [--inner K] [--threads N] [--loop-samples N] [--shapes 32:882:22,...] [--out PATH]"""
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
import vt_synth_fp64 as R  # noqa: E402
from artspeech_amd import vocal_tract_synthesis as V  # noqa: E402
from bench_synthesis import host_ms, spread, window_ms  # noqa: E402

T, FRAMERATE, RAGGED = 200, 50, 30


def torch_loop(areas, sections, source, S, n, r_g=R.R_GLOTTIS, r_l=R.R_LIPS, mu=R.MU, min_area=R.MIN_AREA):
    """The first n output samples (B, n) of the differenced ladder by stock torch ops, one sample per round of launches; every
    utterance has sections[0] sections (the benchmark's batches do)."""
    K = int(sections[0])
    A = areas[:, :, :K].clamp(min=min_area)
    kf = (A[:, :, :-1] - A[:, :, 1:]) / (A[:, :, :-1] + A[:, :, 1:])
    B = A.shape[0]
    Rw = torch.zeros((B, K), dtype=torch.float64, device=areas.device)
    Lw = torch.zeros_like(Rw)
    out = torch.zeros((B, n), dtype=torch.float64, device=areas.device)
    y_prev = torch.zeros(B, dtype=torch.float64, device=areas.device)
    last = A.shape[1] - 1
    for i in range(n):
        t, s = divmod(i, S)
        k = kf[:, t] + (kf[:, min(t + 1, last)] - kf[:, t]) * (s / S)
        y = (1 + r_l) * Rw[:, K - 1]
        out[:, i] = y - y_prev
        y_prev = y
        w = k * (Rw[:, :-1] - Lw[:, 1:])
        Rn = torch.cat([(mu * (source[:, i] + r_g * Lw[:, 0]))[:, None], mu * (Rw[:, :-1] + w)], 1)
        Lw = torch.cat([mu * (Lw[:, 1:] + w), (mu * (r_l * Rw[:, K - 1]))[:, None]], 1)
        Rw = Rn
    return out


def host_loop(areas, sections, frames, S, source, n, threads):
    """The restatement on the first n samples (frames cut to what n needs), the utterances split over the threads."""
    need = -(-n // S) + 1
    chunks = [c for c in np.array_split(np.arange(len(areas)), threads) if len(c)]
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda c: R.ladder(areas[c][:, :need], sections[c], np.minimum(frames[c], need), S,
                                                 source[c][:, :need * S])[0][:, :n], chunks))
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--loop-samples", type=int, default=2000)
    ap.add_argument("--shapes", default="32:882:22,4:882:22,32:1764:44", help="comma-separated B:S:K")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vt_synth_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vt_synth needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    n_loop = args.loop_samples
    result = {"T": T, "framerate": FRAMERATE, "ragged_sections": RAGGED, "device": torch.cuda.get_device_name(0), "cpu_threads": args.threads,
              "repeats": args.repeats, "inner": args.inner, "loop_samples": n_loop,
              "kernel_time_alone_ms": "not measured (the windows hold the launch and as_vt_waveguide's read-back of the section counts)",
              "shapes": {}}
    for B, S, K in [tuple(int(v) for v in shape.split(":")) for shape in args.shapes.split(",")]:
        fs = float(S * FRAMERATE)
        rng = np.random.default_rng([B, S, K])
        # ragged sections of a tube K c / fs long, areas that drift from frame to frame with a constriction that comes and goes
        lengths_h = rng.uniform(0.5, 1.5, (B, T, RAGGED))
        lengths_h *= (K * R.SOUND_SPEED / fs) / lengths_h.sum(-1, keepdims=True)
        areas_h = np.exp(0.6 * rng.standard_normal((B, 1, RAGGED)) + 0.3 * np.cumsum(rng.standard_normal((B, T, RAGGED)), 1) / np.sqrt(T))
        areas_h[:, T // 3:T // 2, RAGGED // 2] = 0.05
        counts_h = np.full((B, T), RAGGED, np.int32)
        frames_h = np.full(B, T, np.int32)
        voicing_h = (rng.uniform(size=(B, T)) < 0.7).astype(np.float64)
        areas, lengths, voicing = (torch.from_numpy(x).to(dev) for x in (areas_h, lengths_h, voicing_h))
        counts, frames = torch.from_numpy(counts_h).to(dev), torch.from_numpy(frames_h).to(dev)
        eq = V.equal_sections(areas, lengths, counts, frames, fs)
        assert eq.sections.tolist() == [K] * B, eq.sections.tolist()
        where, gain = V.frication_control(eq.areas, eq.sections, 0.1)
        f0 = torch.linspace(120.0, 90.0, T, dtype=torch.float64, device=dev)[None, :].repeat(B, 1)
        source, _ = V.glottal_source(f0, voicing, 0.05 * (1 - voicing), frames, S, fs)
        variants = (("hip_ladder", lambda: V.waveguide(eq.areas, eq.sections, frames, S, source, where, gain, out64=False)),
                    ("hip_source", lambda: V.glottal_source(f0, voicing, 0.05 * (1 - voicing), frames, S, fs)),
                    ("hip_end_to_end", lambda: V.synthesize_speech(areas, lengths, counts, voicing, frames, S, FRAMERATE)))
        for _ in range(2):   # warm-up of every variant at the timed shape
            for _, fn in variants:
                fn()
        t = {name: [] for name, _ in variants}
        for _ in range(args.repeats):   # alternating windows of the same run
            for name, fn in variants:
                t[name].append(window_ms(fn, args.inner))
        torch_loop(eq.areas, eq.sections, source, S, 50)   # warm-up
        t_torch = host_ms(lambda: torch_loop(eq.areas, eq.sections, source, S, n_loop), 1)
        eq_h, sections_h, source_h = eq.areas.cpu().numpy(), eq.sections.cpu().numpy(), source.cpu().numpy()
        t_host = host_ms(lambda: host_loop(eq_h, sections_h, frames_h, S, source_h, n_loop, args.threads), 1)
        # parity on the first samples, without frication (the torch loop has none)
        plain = V.waveguide(eq.areas, eq.sections, frames, S, source, out32=False).out64[:, :n_loop]
        by_torch = torch_loop(eq.areas, eq.sections, source, S, n_loop)
        by_host = host_loop(eq_h, sections_h, frames_h, S, source_h, n_loop, args.threads)
        scale = float(np.abs(by_host).max())
        med = {name: float(np.median(v)) for name, v in t.items()}
        samples = T * S
        entry = {f"{name}_ms": spread(v) for name, v in t.items()}
        entry.update(B=B, S=S, K=K, sample_rate=fs, samples_per_utterance=samples, audio_seconds=B * T / FRAMERATE,
                     audio_seconds_per_second_of_ladder=(B * T / FRAMERATE) / (med["hip_ladder"] * 1e-3),
                     ns_per_recurrent_step=med["hip_ladder"] * 1e6 / samples,
                     end_to_end_over_ladder=med["hip_end_to_end"] / med["hip_ladder"],
                     torch_loop={"measured_ms": t_torch, "measured_samples": n_loop, "scaled_ms": t_torch * samples / n_loop,
                                 "note": "timed on measured_samples samples and scaled to T S; not run in full"},
                     host_loop={"measured_ms": t_host, "measured_samples": n_loop, "scaled_ms": t_host * samples / n_loop,
                                "note": "timed on measured_samples samples and scaled to T S; not run in full"},
                     torch_loop_scaled_over_hip_ladder=t_torch * samples / n_loop / med["hip_ladder"],
                     host_loop_scaled_over_hip_ladder=t_host * samples / n_loop / med["hip_ladder"],
                     max_rel_diff_hip_torch=float((plain - by_torch).abs().max()) / scale,
                     max_rel_diff_hip_host=float(np.abs(plain.cpu().numpy() - by_host).max()) / scale)
        result["shapes"][f"B{B}-S{S}-K{K}"] = entry
        print(json.dumps({f"B{B}-S{S}-K{K}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
