#!/usr/bin/env python
"""Cost of the forced alignment (as_ctc_align) at the recogniser-evaluation shape of tools/bench_recognizer_eval.py: one batch of the
seeded synthetic data set, T = 200 frames, C = 45 classes, collapsed targets of about 50 labels, at B = 32 and B = 4, on
"trained-like" emissions (the per-frame targets one-hot, 25 % of the frames turned to blank, plus noise).

as_ctc_align (recursion, trace-back and expansion into every output, one launch) is timed against two comparators, in alternating
windows of the same run:

  (a) as_ctc_loss with with_beta = 0 on the same inputs: the sum-recursion over the same trellis, alpha only -- the natural floor
      for a time-sequential walk of T steps (it also writes every step's S values to its workspace, which the alignment does not);
  (b) a straightforward host loop: the emissions copied to the host, then per utterance a numpy Viterbi over the same state graph
      with the same tie rules and a Python trace-back.

Device calls are timed with events around `iters` back-to-back calls on preallocated buffers (no allocation, no synchronise
inside the window); the host loop with a host clock, its download included.  Both input modes are timed: log-probabilities, and
logits (the alignment normalises inside its one launch; the loss launches its row-logsumexp kernel first).  The alignment's scores
must equal the host loop's on these inputs to 1e-3 (fp32 against fp64 sums of 200 terms).

    python tools/bench_forced_align.py [--iters N] [--warmup W] [--rounds R] [--out profiles/forced_align_bench.json]

Per-kernel times: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_forced_align.py --rounds 1` (the kernels are
ctc_align_kernel, ctc_alpha_beta_kernel, ctc_row_lse_kernel)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def host_viterbi(logp, target, blank):
    """(score, frame_filled) of one utterance on the host, float64: stay, step, skip in that order, strictly greater wins, the
    label state wins the end"""
    Tb, L = logp.shape[0], len(target)
    S = 2 * L + 1
    ext = np.full(S, blank)
    ext[1::2] = target
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    a = np.full(S, -np.inf)
    a[: min(2, S)] = logp[0, ext[: min(2, S)]]
    back = np.zeros((Tb, S), dtype=np.int8)
    for t in range(1, Tb):
        step = np.concatenate([[-np.inf], a[:-1]])
        skp = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]])[:S], -np.inf)
        bp = (step > a).astype(np.int8)
        best = np.maximum(a, step)
        m = skp > best
        back[t] = np.where(m, 2, bp)
        a = np.where(m, skp, best) + logp[t, ext]
    s = S - 2 if S >= 2 and a[S - 2] >= a[S - 1] else S - 1
    score = a[s]
    filled = np.zeros(Tb, dtype=np.int32)
    for t in range(Tb - 1, -1, -1):
        filled[t] = s // 2 if s % 2 else max(s // 2 - 1, 0)
        s -= back[t, s]
    return score, filled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition import Feature, forced_align
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    from train_phoneme_recognition import Criterion, build_vocabulary

    dev = torch.device("cuda", 0)
    T = 200
    vocabulary = build_vocabulary(None, Criterion.CTC)
    C = len(vocabulary)
    results, summary = [], {}
    for B in (32, 4):
        ds = SyntheticPhonemeRecognitionDataset(B, vocabulary, min_len=T, max_len=T, seed=0)
        batch = collate_fn([ds[i] for i in range(B)], [Feature.VOCAL_TRACT])
        il_h, tl_h = batch["vocal_tract_length"], batch["ctc_target_length"]
        targets = batch["ctc_target"].to(dev).contiguous()
        g = torch.Generator().manual_seed(1)
        frames = batch["articulatory_target"]
        hot = torch.where(torch.rand(B, T, generator=g) < 0.25, torch.zeros_like(frames), frames)
        scores = (6.0 * torch.nn.functional.one_hot(hot, C).float() + torch.randn(B, T, C, generator=g)).to(dev)
        il, tl, max_l = il_h.to(dev), tl_h.to(dev), int(tl_h.max())
        ws_align = int(_lib.call("as_ctc_align_workspace_bytes", T, B, max_l))
        ws_a = torch.empty(max(ws_align, 1), device=dev, dtype=torch.uint8)
        wsn = int(_lib.call("as_ctc_workspace_floats", T, B, max_l))
        ws_l = torch.empty(wsn, device=dev)
        score, nll = torch.empty(B, device=dev), torch.empty(B, device=dev)
        fr = torch.empty(3, B, T, device=dev, dtype=torch.int32)
        spans, span_score = torch.empty(B, max_l, 2, device=dev, dtype=torch.int32), torch.empty(B, max_l, device=dev)
        for mode, x in (("log_probs", torch.log_softmax(scores, -1)), ("logits", scores)):
            lg = int(mode == "logits")

            def align():
                _lib.call("as_ctc_align", x, x.stride(1), x.stride(0), T, B, C, lg, targets, targets.shape[1], il, tl, max_l, 0,
                          ws_a if ws_align else None, ws_align, score, fr[0], fr[1], fr[2], spans, span_score)

            def loss():
                _lib.call("as_ctc_loss", x, x.stride(1), x.stride(0), T, B, C, lg, targets, targets.shape[1], il, tl, max_l, 0, 0,
                          ws_l, wsn, nll)

            def host():
                lp = (torch.log_softmax(x, -1) if lg else x).cpu().double().numpy()
                tg = targets.cpu().numpy()
                return [host_viterbi(lp[b, : int(il_h[b])], tg[b, : int(tl_h[b])], 0) for b in range(B)]

            ref = host()
            al = forced_align(x, targets, il_h, tl_h, 0, logits=bool(lg))
            got, filled = al.score.cpu().numpy(), al.frame_filled.cpu().numpy()
            assert al.feasible.all() and max(abs(float(a) - r[0]) for a, r in zip(got, ref)) < 1e-3
            same_frames = float(np.mean([np.mean(filled[b, : len(r[1])] == r[1]) for b, r in enumerate(ref)]))

            def window(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.iters   # us per call

            for _ in range(args.warmup):
                align(), loss()
            torch.cuda.synchronize()
            t_align, t_loss, t_host = [], [], []
            for r in range(args.rounds):   # alternating windows
                t_align.append(window(align))
                t_loss.append(window(loss))
                if r < 3:
                    t0 = time.perf_counter()
                    host()
                    t_host.append((time.perf_counter() - t0) * 1e6)
            med = lambda v: float(sorted(v)[len(v) // 2])   # noqa: E731
            row = dict(workload=f"forced_align_B{B}_T{T}_C{C}", mode=mode, mean_target_labels=round(float(tl_h.float().mean()), 1),
                       max_target_labels=max_l, workspace_bytes=ws_align,
                       align_us=dict(median=round(med(t_align), 2), min=round(min(t_align), 2), max=round(max(t_align), 2)),
                       ctc_alpha_us=dict(median=round(med(t_loss), 2), min=round(min(t_loss), 2), max=round(max(t_loss), 2)),
                       host_loop_us=dict(median=round(med(t_host), 1), min=round(min(t_host), 1), max=round(max(t_host), 1)),
                       align_over_ctc_alpha=round(med(t_align) / med(t_loss), 3), host_loop_over_align=round(med(t_host) / med(t_align), 1),
                       frames_equal_to_host_loop=round(same_frames, 4), iters=args.iters, rounds=args.rounds)
            print(json.dumps(row), flush=True)
            results.append(row)
            summary[f"B{B}_{mode}"] = dict(align_over_ctc_alpha=row["align_over_ctc_alpha"], host_loop_over_align=row["host_loop_over_align"])
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"workload": f"forced alignment of one synthetic batch, T={T}, C={C}, collapsed targets, B=32 and B=4",
                       "command": "python tools/bench_forced_align.py --out FILE", "device": torch.cuda.get_device_name(0),
                       "timing": "device events around `iters` back-to-back calls per window, alternating windows; host loop: host clock",
                       "timings": results, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
