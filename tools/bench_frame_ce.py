"""The frame-level criterion and metrics at the thesis shape (T = 200, C = 45, ragged lengths) for B = 32 and B = 4.  All timings
come from one run, alternating per repeat:
  hip_ce        frame_cross_entropy on the permuted view of the (B, T, C) logits + backward (as_frame_ce_loss, as_frame_ce_grad and
                the torch glue between them); device events around `inner` calls in a row, a synchronise on both sides of the window
  torch_ce      the reference's path in stock torch on the same GPU: pad masks from a cumsum, boolean gathers of the valid rows and
                targets, F.cross_entropy, autograd backward to the logits; timed the same way
  hip_auroc     metrics.AUROC on device probabilities (as_frame_auroc, one download of 3 C integers); host clock around a call that
  hip_accuracy  ends on the host, as does metrics.Accuracy (as_decode_top1 + as_confusion_counts, one download of C * C integers)
  host_auroc    the host path: download of the emissions, boolean gathers, sklearn.metrics.roc_auc_score per class that has both
  host_accuracy kinds of frame / recall_score(average="macro") on `--threads` CPU threads; host clock
The two criteria are also compared (loss and largest gradient difference) and so are the metric values.  No time is a pass
criterion.  Writes profiles/frame_ce_bench.json.
usage: python tools/bench_frame_ce.py [--repeats R] [--inner K] [--threads N] [--batches 32,4] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_recognition import frame_cross_entropy  # noqa: E402
from artspeech_amd.phoneme_recognition.metrics import AUROC, Accuracy  # noqa: E402

T, C = 200, 45


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


def host_ms(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def pad_mask(B, time_steps, lengths, device):
    """MetricsMixin.get_pad_mask: built on the host from a cumsum, then moved"""
    cumsum = torch.cumsum(torch.ones((B, time_steps)), dim=1)
    return (cumsum <= lengths.repeat(time_steps, 1).T).type(torch.long).to(device)


def torch_ce(logits, targets, lengths):
    """CrossEntropyLoss.forward of the reference on (B, T, C) logits, and its backward"""
    B = logits.shape[0]
    logits.grad = None
    em_mask = torch.flatten(pad_mask(B, logits.shape[1], lengths, logits.device))
    tg_mask = torch.flatten(pad_mask(B, targets.shape[1], lengths, logits.device))
    rows = torch.flatten(logits, 0, 1)[em_mask == 1]
    y = torch.flatten(targets, 0, 1)[tg_mask == 1]
    loss = torch.nn.functional.cross_entropy(rows, y)
    loss.backward()
    return loss.detach()


def hip_ce(logits, targets, lengths):
    logits.grad = None
    loss = frame_cross_entropy(logits.permute(1, 0, 2), targets, lengths, lengths)
    loss.backward()
    return loss.detach()


def gathered(probs, targets, lengths):
    probs, targets = probs.cpu(), targets.cpu()
    mask = torch.arange(probs.shape[1])[None, :] < lengths[:, None]
    return probs[mask].numpy(), targets[mask].numpy()


def host_auroc(probs, targets, lengths):
    from sklearn.metrics import roc_auc_score
    rows, y = gathered(probs, targets, lengths)
    per = [roc_auc_score(y == c, rows[:, c]) for c in range(rows.shape[1]) if 0 < (y == c).sum() < len(y)]
    return float(np.mean(per))


def host_accuracy(probs, targets, lengths):
    from sklearn.metrics import recall_score
    rows, y = gathered(probs, targets, lengths)
    pred = rows.argmax(axis=1)
    return float(recall_score(y, pred, labels=sorted(set(y.tolist()) | set(pred.tolist())), average="macro", zero_division=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batches", default="32,4", help="comma-separated batch sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_ce_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_ce needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    result = {"T": T, "C": C, "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "repeats": args.repeats,
              "inner": args.inner, "batches": {}}
    for B in [int(v) for v in args.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        lengths = torch.randint(T // 3, T + 1, (B,), generator=g)
        lengths[0] = T
        logits_a = (3.0 * torch.randn(B, T, C, generator=g)).to(dev).requires_grad_(True)
        logits_b = logits_a.detach().clone().requires_grad_(True)
        targets = torch.randint(0, C, (B, T), generator=g).to(dev)
        probs = torch.softmax(logits_a.detach(), dim=-1)
        auroc, accuracy = AUROC(C), Accuracy(C)
        variants = (("hip_ce", window_ms, lambda: hip_ce(logits_a, targets, lengths)),
                    ("torch_ce", window_ms, lambda: torch_ce(logits_b, targets, lengths)),
                    ("hip_auroc", host_ms, lambda: auroc(probs, targets, lengths, lengths)),
                    ("host_auroc", host_ms, lambda: host_auroc(probs, targets, lengths)),
                    ("hip_accuracy", host_ms, lambda: accuracy(probs, targets, lengths, lengths)),
                    ("host_accuracy", host_ms, lambda: host_accuracy(probs, targets, lengths)))
        values = {}
        for _ in range(3):   # warm-up of every variant at the timed shape
            values = {name: fn() for name, _, fn in variants}
        t = {name: [] for name, _, _ in variants}
        for _ in range(args.repeats):   # alternating windows of the same run
            for name, clock, fn in variants:
                t[name].append(clock(fn, args.inner if clock is window_ms else max(1, args.inner // 10)))
        med = {name: float(np.median(v)) for name, v in t.items()}
        entry = {f"{name}_ms": spread(v) for name, v in t.items()}
        entry.update(valid_frames=int(lengths.sum()),
                     torch_over_hip_ce_at_median=med["torch_ce"] / med["hip_ce"],
                     host_over_hip_auroc_at_median=med["host_auroc"] / med["hip_auroc"],
                     host_over_hip_accuracy_at_median=med["host_accuracy"] / med["hip_accuracy"],
                     loss_hip=float(values["hip_ce"]), loss_torch=float(values["torch_ce"]),
                     max_abs_grad_diff=float((logits_a.grad - logits_b.grad).abs().max()),
                     auroc_hip=float(values["hip_auroc"]), auroc_host=values["host_auroc"],
                     accuracy_hip=float(values["hip_accuracy"]), accuracy_host=values["host_accuracy"])
        result["batches"][f"B{B}"] = entry
        print(json.dumps({f"B{B}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
