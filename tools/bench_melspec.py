"""The log-mel front end at the thesis parameters (16 kHz, n_fft 1024, win_length 1024, hop_length 256, 80 mels, 2 channels) on
batches of 4 s utterances, B = 4 (the thesis's batch) and B = 32.  All timings come from one run, alternating per repeat:
  fused       MelSpectrogram.log_mel_batch (one as_melspec_fwd launch) from waveforms already on the device to the collated
              (B, 2, 80, T) batch; device events around `inner` calls in a row, a synchronise on both sides of the window
  stock_gpu   the same result from stock torch on the same GPU: torch.stft -> abs().pow(2) -> matmul with the filterbank ->
              log(clamp) -> the copy into both planes of a -1 filled batch; timed the same way.  The utterances are equally long,
              which is the stock path's best case (one batched stft, no per-item loop)
  host_items  the reference's per-item path on the host: per utterance the signal copied to two channels, torch.stft, power,
              filterbank, log(clamp) in float32 on `--threads` CPU threads, then pad_sequence; host clock
and the algorithmic bytes (waveforms in + features out) over the fused time beside a plain device copy of as many bytes.
No time is a pass criterion.  Writes profiles/melspec_bench.json.
usage: python tools/bench_melspec.py [--seconds S] [--repeats R] [--inner K] [--threads N] [--batches 4,32] [--out PATH]"""
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
from artspeech_amd.phoneme_recognition.features import MelSpectrogram  # noqa: E402

PARAMS = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop_length=256, n_mels=80)
CLIP = 1e-5


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


def stock_log_mel(waves, window, fbanks, channels=2):
    spec = torch.stft(waves, PARAMS["n_fft"], hop_length=PARAMS["hop_length"], win_length=PARAMS["win_length"], window=window,
                      center=True, pad_mode="reflect", return_complex=True)
    mel = torch.matmul(spec.abs().pow(2).transpose(-1, -2), fbanks).transpose(-1, -2)
    logmel = torch.log(torch.clamp(mel, min=CLIP))
    out = torch.full((waves.shape[0], channels, logmel.shape[-2], logmel.shape[-1]), -1.0, dtype=logmel.dtype, device=logmel.device)
    out[:] = logmel[:, None]
    return out


def host_items(signals, window, fbanks):
    feats = []
    for x in signals:
        audio = torch.cat([x[None], x[None]], dim=0)   # mono to stereo
        spec = torch.stft(audio, PARAMS["n_fft"], hop_length=PARAMS["hop_length"], win_length=PARAMS["win_length"], window=window,
                          center=True, pad_mode="reflect", return_complex=True)
        mel = torch.matmul(spec.abs().pow(2).transpose(-1, -2), fbanks).transpose(-1, -2)
        feats.append(torch.log(torch.clamp(mel, min=CLIP)).permute(2, 0, 1))
    return pad_sequence(feats, batch_first=True, padding_value=-1).permute(0, 2, 3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batches", default="4,32", help="comma-separated batch sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melspec_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_melspec needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    ms = MelSpectrogram(**PARAMS)
    n = int(args.seconds * PARAMS["sample_rate"])
    result = {"params": PARAMS, "seconds": args.seconds, "samples": n, "device": torch.cuda.get_device_name(0),
              "cpu_threads": torch.get_num_threads(), "repeats": args.repeats, "inner": args.inner, "batches": {}}
    window_dev, fbanks_dev = ms.window.to(dev), ms.fbanks.to(dev)
    for B in [int(v) for v in args.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        host_waves = 0.3 * torch.randn(B, n, generator=g)
        waves, lengths = host_waves.to(dev), torch.full((B,), n, dtype=torch.int64)
        fused = lambda: ms.log_mel_batch(waves, lengths)                      # noqa: E731
        stock = lambda: stock_log_mel(waves, window_dev, fbanks_dev)          # noqa: E731
        a, b = fused()[0], stock()
        for _ in range(3):
            fused(), stock()
        t_fused, t_stock = [], []
        for _ in range(args.repeats):   # alternating windows of the same run
            t_fused.append(window_ms(fused, args.inner))
            t_stock.append(window_ms(stock, args.inner))
        nbytes = waves.numel() * 4 + a.numel() * 4
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        t_copy = [window_ms(lambda: dst.copy_(src), args.inner) for _ in range(args.repeats)]   # reads and writes nbytes / 2 each
        signals = list(host_waves)
        host_items(signals[:2], ms.window, ms.fbanks)
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter()
            c = host_items(signals, ms.window, ms.fbanks)
            t_host.append((time.perf_counter() - t0) * 1e3)
        entry = {"frames": int(a.shape[-1]), "fused_ms": spread(t_fused), "stock_gpu_ms": spread(t_stock), "host_items_ms": spread(t_host),
                 "stock_over_fused_at_median": float(np.median(t_stock) / np.median(t_fused)),
                 "algorithmic_bytes": nbytes, "fused_GB_per_s_at_median": nbytes / np.median(t_fused) / 1e6,
                 "plain_copy_ms": spread(t_copy), "plain_copy_GB_per_s_at_median": nbytes / np.median(t_copy) / 1e6,
                 "stock_spectrum_bytes": int(B * 513 * a.shape[-1] * 8),
                 "max_abs_diff_fused_vs_stock_gpu": float((a - b).abs().max()),
                 "max_abs_diff_fused_vs_host_items": float((a.cpu() - c).abs().max())}
        result["batches"][f"B{B}"] = entry
        print(json.dumps({f"B{B}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
