"""The result tables of a test pass at the thesis shape (100 sentences x 200 frames x 11 articulators, N = 50), three ways on the
same machine, each a host clock around work that ends in a device synchronise or on the host (median / min / max over the repeats
after a warm-up; `runs` says how many each path got):
  in_memory   ErrorReport fed by batches of 16 padded sentences that are already on the device, as a test loop feeds it (the
              per-frame metric kernels included), then write(): statistics, one copy, the four files
  from_files  report_from_results_dir's steps on a tree of contour dumps: reading (np.load + csv, host only) and the device part
              (upload, kernels, write()) timed separately
  host        the path the reference takes, restated with stock PyTorch and pandas on the CPU: the two metrics on a 1 x 1 batch
              per frame (torch.cdist -> min -> mean; sqrt of the squared differences), a row dict per frame and articulator,
              DataFrame.groupby("articulator").agg and groupby("sentence").corr per tract variable; the .npy reads it also does
              are the `reading` figure of from_files
The tract variables are seeded random numbers (their kernel is not what is timed).  No pass mark is set on these times.
Writes profiles/report_bench.json.
usage: python tools/bench_report.py [--sentences S] [--frames T] [--repeats R] [--host-repeats H] [--out PATH]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation.report import ErrorReport, read_sentence  # noqa: E402
from artspeech_amd.settings import DATASET_CONFIG  # noqa: E402
from artspeech_amd.tract_variables import TV_NAMES  # noqa: E402

ARTICULATORS = ["arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate-midline", "thyroid-cartilage",
                "tongue", "upper-incisor", "upper-lip", "vocal-folds"]
N, BATCH = 50, 16


def spread(times):
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def tv_text(name, frames, phonemes, tv_pred, tv_target):
    """A per-sentence tract_variables.csv with the columns the report reads."""
    lines = [",".join(["sentence", "frame", "phoneme", *(f"{v}_target" for v in TV_NAMES), *(f"{v}_pred" for v in TV_NAMES)])]
    for f, p, t, q in zip(frames, phonemes, tv_target, tv_pred):
        lines.append(",".join([name, f, p, *(repr(float(v)) for v in t), *(repr(float(v)) for v in q)]))
    return "\n".join(lines) + "\n"


def make_case(S, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(S, T, len(ARTICULATORS), 2, N, generator=g)
    true = pred + 0.05 * torch.randn(S, T, len(ARTICULATORS), 2, N, generator=g)
    tv_target = torch.rand(S, T, 4, generator=g) * 0.1
    tv_pred = tv_target + 0.02 * torch.randn(S, T, 4, generator=g)
    names = [f"sent{s:03d}" for s in range(S)]
    frames = [[f"{t:04d}" for t in range(T)] for _ in range(S)]
    phonemes = [[f"ph{(s + t // 7) % 43:02d}" for t in range(T)] for s in range(S)]
    texts = [tv_text(names[s], frames[s], phonemes[s], tv_pred[s], tv_target[s]) for s in range(S)]
    return pred, true, tv_pred, tv_target, names, frames, phonemes, texts


def write_tree(root, case):
    pred, true, _, _, names, frames, _, texts = case
    for s, name in enumerate(names):
        d = os.path.join(root, "test_outputs", "0", name)
        os.makedirs(os.path.join(d, "contours"))
        with open(os.path.join(d, "tract_variables.csv"), "w", newline="") as f:
            f.write(texts[s])
        p, t = pred[s].numpy(), true[s].numpy()
        for i, frame in enumerate(frames[s]):
            for a, art in enumerate(ARTICULATORS):
                np.save(os.path.join(d, "contours", f"{frame}_{art}.npy"), p[i, a])
                np.save(os.path.join(d, "contours", f"{frame}_{art}_true.npy"), t[i, a])


def in_memory(case, dev, cfg, out_dir):
    pred, true, tv_pred, tv_target, names, frames, phonemes, texts = case
    S, T = pred.shape[:2]
    batches = [(pred[s:s + BATCH].to(dev), true[s:s + BATCH].to(dev), tv_pred[s:s + BATCH].to(dev), tv_target[s:s + BATCH].to(dev))
               for s in range(0, S, BATCH)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    report = ErrorReport(ARTICULATORS, cfg, dev)
    for k, (p, t, vp, vt) in enumerate(batches):
        s = k * BATCH
        report.add(p, t, [T] * p.shape[0], names[s:s + BATCH], frames[s:s + BATCH], phonemes[s:s + BATCH],
                   tv=(vp, vt, texts[s:s + BATCH]))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    report.write(out_dir)
    t2 = time.perf_counter()
    return {"add_ms": (t1 - t0) * 1e3, "write_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}


def from_files(root, dev, cfg, out_dir):
    base = os.path.join(root, "test_outputs", "0")
    reading = device = 0.0
    report = ErrorReport(ARTICULATORS, cfg, dev)
    torch.cuda.synchronize()
    for name in sorted(os.listdir(base)):
        t0 = time.perf_counter()
        text, frames, phonemes, outputs, targets, vp, vt = read_sentence(os.path.join(base, name), ARTICULATORS)
        t1 = time.perf_counter()
        report.add(outputs.to(dev), targets.to(dev), [len(frames)], [name], [frames], [phonemes], tv=(vp.to(dev), vt.to(dev), [text]))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        reading, device = reading + (t1 - t0), device + (t2 - t1)
    t0 = time.perf_counter()
    report.write(out_dir)
    device += time.perf_counter() - t0
    return {"reading_ms": reading * 1e3, "device_and_write_ms": device * 1e3, "total_ms": (reading + device) * 1e3}


def host_reference(case, to_mm, out_dir):
    """The reference's computation (report_phoneme_to_articulation.py:198-285) on contours already in memory."""
    import pandas as pd
    pred, true, tv_pred, tv_target, names, frames, phonemes, _ = case
    S, T = pred.shape[:2]
    t0 = time.perf_counter()
    rows = []
    for s in range(S):
        for f in range(T):
            p, t = pred[s, f][None, None], true[s, f][None, None]                     # (1, 1, A, 2, N)
            d = torch.cdist(p.transpose(-1, -2), t.transpose(-1, -2))
            p2cp = ((d.min(dim=-1).values.sum(dim=-1) / N + d.min(dim=-2).values.sum(dim=-1) / N) / 2)[0, 0]
            euclid = torch.sqrt((p[..., 0, :] - t[..., 0, :]) ** 2 + (p[..., 1, :] - t[..., 1, :]) ** 2).mean(dim=-1)[0, 0]
            for a, art in enumerate(ARTICULATORS):
                rows.append({"sentence_name": names[s], "frame": int(frames[s][f]), "phoneme": phonemes[s][f], "articulator": art,
                             "p2cp": p2cp[a].item(), "p2cp_mm": p2cp[a].item() * to_mm, "euclidean": euclid[a].item(),
                             "euclidean_mm": euclid[a].item() * to_mm})
    t1 = time.perf_counter()
    df = pd.DataFrame(rows)
    df.to_csv(os.path.join(out_dir, "error_report_full.csv"), index=False)
    stats = ["mean", "std", "min", "max"]
    df.groupby("articulator").agg({k: stats for k in ("p2cp", "p2cp_mm", "euclidean", "euclidean_mm")}).reset_index().to_csv(
        os.path.join(out_dir, "error_report_agg.csv"), index=False)
    tv = pd.DataFrame({"sentence": [n for n in names for _ in range(T)]})
    data = []
    for j, name in enumerate(TV_NAMES):
        tv[f"{name}_target"], tv[f"{name}_pred"] = tv_target[..., j].reshape(-1).double().numpy() * to_mm, tv_pred[..., j].reshape(-1).double().numpy() * to_mm
        c = tv.groupby("sentence")[[f"{name}_target", f"{name}_pred"]].corr().reset_index()
        c = c[c.level_1 == f"{name}_target"][f"{name}_pred"]
        data.append({"TV": name, "mean": c.mean(), "std": c.std(), "min": c.min(), "max": c.max()})
    pd.DataFrame(data).to_csv(os.path.join(out_dir, "TV_corr_report.csv"), index=False)
    t2 = time.perf_counter()
    return {"per_frame_metrics_ms": (t1 - t0) * 1e3, "pandas_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=100)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_report needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    cfg = DATASET_CONFIG["artspeech2"]
    case = make_case(args.sentences, args.frames)
    tmp = tempfile.mkdtemp(prefix="bench_report_")
    try:
        tree = os.path.join(tmp, "tree")
        t0 = time.perf_counter()
        write_tree(tree, case)
        print(f"wrote the tree in {time.perf_counter() - t0:.1f} s", flush=True)
        out = {k: os.path.join(tmp, k) for k in ("memory", "files", "host")}
        os.makedirs(out["host"])
        result = {"shape": {"sentences": args.sentences, "frames_per_sentence": args.frames, "articulators": len(ARTICULATORS),
                            "n_samples": N, "batch": BATCH}, "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
                  "repeats": args.repeats}
        for name, fn in (("in_memory", lambda: in_memory(case, dev, cfg, out["memory"])),
                         ("from_files", lambda: from_files(tree, dev, cfg, out["files"])),
                         ("host", lambda: host_reference(case, cfg.RES * cfg.PIXEL_SPACING, out["host"]))):
            if name == "host":   # warm-up on one sentence (operator set-up, pandas imports); the full pass takes seconds
                host_reference(tuple(c[:1] for c in case), cfg.RES * cfg.PIXEL_SPACING, out["host"])
            else:
                fn()   # warm-up: code objects, the file cache
            runs = [fn() for _ in range(args.repeats if name != "host" else args.host_repeats)]
            result[name] = {k: spread([r[k] for r in runs]) for k in runs[0]}
            result[name]["runs"] = len(runs)
            print(json.dumps({name: result[name]}), flush=True)
        with open(os.path.join(out["memory"], "error_report_agg.csv")) as a, open(os.path.join(out["files"], "error_report_agg.csv")) as b:
            result["both_device_paths_write_the_same_agg"] = a.read() == b.read()
        result["speedup_in_memory_vs_host"] = result["host"]["total_ms"]["median"] / result["in_memory"]["total_ms"]["median"]
        result["speedup_from_files_vs_host_plus_reading"] = (
            (result["host"]["total_ms"]["median"] + result["from_files"]["reading_ms"]["median"]) / result["from_files"]["total_ms"]["median"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
