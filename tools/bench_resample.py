"""The resampler ahead of the log-mel at 44.1 kHz -> 16 kHz (Hann window, torchaudio's defaults) on batches of 4 s utterances,
B = 4 (the thesis's batch) and B = 32.  All timings come from one run, alternating per repeat:
  banded      Resample.resample_batch (one as_resample_fwd launch) from float32 waveforms already on the device to the padded
              (B, m) batch at 16 kHz; device events around `inner` calls in a row, a synchronise on both sides of the window.
              banded_int16 is the same launch from int16 samples
  dense_gpu   what the stock formulation runs, in stock torch on the same GPU: the waveforms zero-padded by (width, width + o),
              torch.nn.functional.conv1d with stride o over the full (n, 1, 2 width + o) table, the transpose to sample order and
              the cut to the new length; timed the same way.  Equally long utterances: the stock path's best case
  host_items  the per-item path on the host: the same dense convolution per utterance in float32 on `--threads` CPU threads, then
              pad_sequence; host clock
  chain       resample_batch + MelSpectrogram.log_mel_batch at the thesis parameters (two launches on one stream) beside
              log_mel_batch alone on waveforms that are already at 16 kHz and as long as the resampled ones
and the algorithmic bytes (waveforms in + waveforms out) over the banded time beside a plain device copy of as many bytes.
No time is a pass criterion.  Writes profiles/resample_bench.json.
usage: python tools/bench_resample.py [--seconds S] [--repeats R] [--inner K] [--threads N] [--batches 4,32] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_recognition.features import MelSpectrogram, Resample, sinc_resample_kernel  # noqa: E402

ORIG, NEW = 44100, 16000
MEL = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop_length=256, n_mels=80)


def spread(times):
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def window_ms(fn, inner):
    """per-call milliseconds of `inner` calls in a row: device events, a synchronise before and after the window"""
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / inner


def dense_resample(waves, table, width, o, new_length):
    """(B, new_length) by the dense strided convolution: table (n, 1, 2 width + o), waves (B, L)"""
    padded = torch.nn.functional.pad(waves, (width, width + o))
    y = torch.nn.functional.conv1d(padded[:, None], table, stride=o)          # (B, n, J)
    return y.transpose(1, 2).reshape(waves.shape[0], -1)[:, :new_length]


def host_items(signals, table, width, o, new_length):
    return pad_sequence([dense_resample(x[None], table, width, o, new_length)[0] for x in signals], batch_first=True, padding_value=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batches", default="4,32", help="comma-separated batch sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    rs, ms = Resample(ORIG, NEW), MelSpectrogram(**MEL)
    dense, width = sinc_resample_kernel(ORIG, NEW)
    table = dense.float()[:, None].contiguous()
    table_dev = table.to(dev)
    L = int(args.seconds * ORIG)
    m = rs.target_length(L)
    result = {"orig_freq": ORIG, "new_freq": NEW, "phases": rs.n, "step": rs.o, "dense_taps": int(dense.shape[1]), "band": rs.band,
              "tile": rs.tile, "melspec": MEL, "seconds": args.seconds, "samples_in": L, "samples_out": m,
              "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "repeats": args.repeats, "inner": args.inner,
              "batches": {}}
    for B in [int(v) for v in args.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        host_waves = (0.3 * torch.randn(B, L, generator=g)).clamp(-1, 1)
        waves, lengths = host_waves.to(dev), torch.full((B,), L, dtype=torch.int64)
        waves16 = torch.round(waves * 32767).to(torch.int16)
        at_16k, lengths_16k = 0.3 * torch.randn(B, m, generator=g).to(dev), torch.full((B,), m, dtype=torch.int64)
        banded = lambda: rs.resample_batch(waves, lengths)                       # noqa: E731
        banded16 = lambda: rs.resample_batch(waves16, lengths)                   # noqa: E731
        stock = lambda: dense_resample(waves, table_dev, width, rs.o, m)         # noqa: E731
        chain = lambda: ms.log_mel_batch(*rs.resample_batch(waves, lengths))     # noqa: E731
        mel_alone = lambda: ms.log_mel_batch(at_16k, lengths_16k)                # noqa: E731
        a, b = banded()[0], stock()
        for _ in range(3):
            banded(), banded16(), stock(), chain(), mel_alone()
        t = {name: [] for name in ("banded", "banded_int16", "dense_gpu", "chain", "mel_alone")}
        for _ in range(args.repeats):   # alternating windows of the same run
            for name, fn in (("banded", banded), ("banded_int16", banded16), ("dense_gpu", stock), ("chain", chain), ("mel_alone", mel_alone)):
                t[name].append(window_ms(fn, args.inner))
        nbytes = waves.numel() * 4 + a.numel() * 4
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        t_copy = [window_ms(lambda: dst.copy_(src), args.inner) for _ in range(args.repeats)]   # reads and writes nbytes / 2 each
        signals = list(host_waves)
        host_items(signals[:2], table, width, rs.o, m)
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter()
            c = host_items(signals, table, width, rs.o, m)
            t_host.append((time.perf_counter() - t0) * 1e3)
        med = {name: float(np.median(v)) for name, v in t.items()}
        entry = {"banded_ms": spread(t["banded"]), "banded_int16_ms": spread(t["banded_int16"]), "dense_gpu_ms": spread(t["dense_gpu"]),
                 "host_items_ms": spread(t_host), "dense_over_banded_at_median": med["dense_gpu"] / med["banded"],
                 "resample_plus_log_mel_ms": spread(t["chain"]), "log_mel_alone_ms": spread(t["mel_alone"]),
                 "chain_minus_log_mel_alone_ms_at_median": med["chain"] - med["mel_alone"],
                 "algorithmic_bytes": nbytes, "banded_GB_per_s_at_median": nbytes / med["banded"] / 1e6,
                 "plain_copy_ms": spread(t_copy), "plain_copy_GB_per_s_at_median": nbytes / np.median(t_copy) / 1e6,
                 "multiplies_dense_over_banded": float(dense.shape[1] / rs.band),
                 "max_abs_diff_banded_vs_dense_gpu": float((a - b).abs().max()),
                 "max_abs_diff_banded_vs_host_items": float((a.cpu() - c).abs().max())}
        result["batches"][f"B{B}"] = entry
        print(json.dumps({f"B{B}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
