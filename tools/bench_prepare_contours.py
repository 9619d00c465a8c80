"""Contour preparation at the thesis size (49 152 frames x 10 articulators, 3 of them clipped, + 3 references, N = 50):
  prepare     one prepare_contours launch (as_prepare_contours) over contours already on the device, timed with device events
              around `inner` launches in a row (median / min / max over the repeats after a warm-up); achieved GB/s from the bytes
              the algorithm needs, F (A + 3) N 8 read and F (A + 1) N 8 written, beside a plain device copy of as many bytes
  host_loop   what the reference does per (frame, articulator): the restatement's clipping in stock torch ops on the CPU
              (torch.where / cat / F.interpolate, the frame shift), timed on the first 2048 frames with a host clock and SCALED
              to all frames (`scaled_from_frames` says so); the file reads it also does are not included
  statistics  contour_statistics (as_column_mean_std) per articulator against torch.mean / torch.std(dim=0) on the same GPU
No time is a pass criterion.  Writes profiles/prepare_contours_bench.json.
usage: python tools/bench_prepare_contours.py [--frames F] [--host-frames H] [--repeats R] [--inner K] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation import SyntheticRawContours, contour_statistics, prepare_contours  # noqa: E402
from artspeech_amd.phoneme_to_articulation.tail_clipper import clip_thresholds  # noqa: E402
from artspeech_amd.settings import DATASET_CONFIG  # noqa: E402

ARTICULATORS = ["arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate-midline", "thyroid-cartilage",
                "tongue", "upper-lip", "vocal-folds"]
N = 50


def spread(times):
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def device_ms(fn, repeats, inner):
    """per-call milliseconds of fn: device events around `inner` calls, `repeats` times after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / inner)
    return times


def host_clip(name, contour, li, ui, ep, thr):
    """the reference's three methods in stock torch ops on the host, one contour"""
    def resample(points):
        return F.interpolate(points.T.unsqueeze(0), size=50).squeeze(0).T
    if name == "tongue":
        ref = li[li[:, 1].argmax()]
        half2 = contour[25:]
        cut = torch.cat([contour[:25], half2[torch.where(half2[:, 1] < ref[1])]])
        ref = ep[ep[:, 1].argmin()]
        half1 = cut[:25]
        return resample(torch.cat([half1[torch.where(half1[:, 1] < ref[1] + thr[0])], cut[25:]]))
    if name == "lower-lip":
        ref = li[li[:, 1].argmax()]
        half2 = contour[25:]
        cut = resample(torch.cat([contour[:25], half2[torch.where(half2[:, 1] < ref[1] + thr[1])]]))
        half1 = cut[:25]
        return resample(torch.cat([half1[torch.where(half1[:, 1] < ref[1])], cut[25:]]))
    if name == "upper-lip":
        ref = ui[-1]
        half2 = contour[25:]
        cut = torch.cat([contour[:25], half2[torch.where(half2[:, 1] > ref[1] - thr[2])]])
        half1 = cut[:25]
        return resample(torch.cat([half1[torch.where(half1[:, 1] > ref[1] - thr[3])], cut[25:]]))
    return contour


def host_loop(raw, refs, thr):
    out = torch.empty(raw.shape[0], raw.shape[1], 2, N)
    for f in range(raw.shape[0]):
        li, ui, ep = refs[f]
        origin = ui.T[:, -1].unsqueeze(-1)
        for a, name in enumerate(ARTICULATORS):
            out[f, a] = (host_clip(name, raw[f, a], li, ui, ep, thr).T - origin) + 0.3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=49152)
    ap.add_argument("--host-frames", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_contours_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prepare_contours needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    cfg = DATASET_CONFIG["artspeech2"]
    data = SyntheticRawContours(args.frames, ARTICULATORS, seed=0)
    A, frames = len(ARTICULATORS), args.frames
    raw, refs = data.raw.to(dev), data.refs.to(dev)
    read_bytes, written_bytes = frames * (A + 3) * N * 8, frames * (A + 1) * N * 8
    result = {"shape": {"frames": frames, "articulators": A, "clipped": 3, "references": 3, "n_samples": N},
              "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "repeats": args.repeats, "inner": args.inner,
              "bytes": {"read": read_bytes, "written": written_bytes}}

    times = device_ms(lambda: prepare_contours(raw, refs, ARTICULATORS, cfg, check=False), args.repeats, args.inner)
    result["prepare"] = {"ms": spread(times), "GB_per_s_at_median": (read_bytes + written_bytes) / np.median(times) / 1e6}
    src = torch.empty(read_bytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty(written_bytes // 4, dtype=torch.float32, device=dev)
    times = device_ms(lambda: dst.copy_(src[:dst.numel()]), args.repeats, args.inner)     # reads and writes `written` bytes
    result["plain_copy"] = {"ms": spread(times), "bytes": 2 * written_bytes, "GB_per_s_at_median": 2 * written_bytes / np.median(times) / 1e6}
    targets, _, counts = prepare_contours(raw, refs, ARTICULATORS, cfg, check=False)
    result["emptied_contours"] = int((counts == 0).sum())
    result["clipped_share"] = {a: float((counts[:, i] < N).float().mean()) for i, a in enumerate(ARTICULATORS) if a in ("tongue", "lower-lip", "upper-lip")}
    print(json.dumps({k: result[k] for k in ("prepare", "plain_copy")}), flush=True)

    h = min(args.host_frames, frames)
    thr = clip_thresholds(cfg)
    host_loop(data.raw[:64], data.refs[:64], thr)   # warm-up: operator set-up
    t0 = time.perf_counter()
    host_out = host_loop(data.raw[:h], data.refs[:h], thr)
    host_ms = (time.perf_counter() - t0) * 1e3
    result["host_loop"] = {"measured_ms": host_ms, "measured_frames": h, "scaled_from_frames": h, "scaled_ms": host_ms * frames / h,
                           "note": "timed on measured_frames frames and scaled linearly to all frames; file reads not included"}
    result["host_loop_equals_device"] = bool(torch.equal(host_out, targets[:h].cpu()))
    result["speedup_vs_scaled_host_loop"] = result["host_loop"]["scaled_ms"] / result["prepare"]["ms"]["median"]
    print(json.dumps({"host_loop": result["host_loop"], "equal": result["host_loop_equals_device"]}), flush=True)

    column = targets[:, 0].contiguous()
    times = device_ms(lambda: contour_statistics(column), args.repeats, args.inner)
    result["statistics"] = {"rows": frames, "cols": 2 * N, "contour_statistics_ms": spread(times)}
    times = device_ms(lambda: (column.mean(dim=0), column.std(dim=0)), args.repeats, args.inner)
    result["statistics"]["torch_mean_std_ms"] = spread(times)
    whole = targets.reshape(frames, -1)
    times = device_ms(lambda: contour_statistics(whole), args.repeats, args.inner)
    result["statistics_all_articulators"] = {"rows": frames, "cols": whole.shape[1], "contour_statistics_ms": spread(times),
                                             "GB_per_s_at_median": whole.numel() * 4 / np.median(times) / 1e6}
    times = device_ms(lambda: (whole.mean(dim=0), whole.std(dim=0)), args.repeats, args.inner)
    result["statistics_all_articulators"]["torch_mean_std_ms"] = spread(times)
    print(json.dumps({k: result[k] for k in ("statistics", "statistics_all_articulators")}), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
