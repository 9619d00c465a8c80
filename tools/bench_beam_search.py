#!/usr/bin/env python
"""Cost of the CTC beam search (as_ctc_beam_search) at the recogniser-evaluation shape of tools/bench_recognizer_eval.py: one batch
of the seeded synthetic data set, B = 32 utterances of T = 200 frames, C = 45 classes, on "trained-like" emissions (the per-frame
targets one-hot, 25 % of the frames turned to blank, plus noise; their log-softmax), at beam 50 and beam 8, merging by max and by
logaddexp, all classes shortlisted, threshold 50, nbest 1.

Best-path decoding (as_decode_top1) is timed beside it on the same emissions, in alternating windows of the same run, so that a
reader sees what the search costs per batch; no time is a pass criterion.  Device calls are timed with events around `iters`
back-to-back calls on preallocated buffers (no allocation, no synchronise inside the window).  The search's best hypothesis
without log_add must be the best path.

    python tools/bench_beam_search.py [--iters N] [--warmup W] [--rounds R] [--out profiles/beam_search_bench.json]

Per-kernel times: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_beam_search.py --rounds 1` (the kernels are
ctc_beam_kernel and the decode kernel of recog_eval.hip)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition import Feature, ctc_beam_search, decode_top1
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    from train_phoneme_recognition import Criterion, build_vocabulary

    dev = torch.device("cuda", 0)
    B, T = 32, 200
    vocabulary = build_vocabulary(None, Criterion.CTC)
    C = len(vocabulary)
    ds = SyntheticPhonemeRecognitionDataset(B, vocabulary, min_len=T, max_len=T, seed=0)
    batch = collate_fn([ds[i] for i in range(B)], [Feature.VOCAL_TRACT])
    lengths = batch["vocal_tract_length"].to(device=dev, dtype=torch.int64)
    g = torch.Generator().manual_seed(1)
    frames = batch["articulatory_target"]
    hot = torch.where(torch.rand(B, T, generator=g) < 0.25, torch.zeros_like(frames), frames)
    x = torch.log_softmax((6.0 * torch.nn.functional.one_hot(hot, C).float() + torch.randn(B, T, C, generator=g)).to(dev), -1)

    tokens = torch.empty(B, 1, T, device=dev, dtype=torch.int32)
    counts, found = torch.empty(B, 1, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    scores = torch.empty(B, 1, device=dev)
    top_tokens, top_counts = torch.empty(B, T, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)

    def top1():
        _lib.call("as_decode_top1", x, x.stride(0), x.stride(1), B, T, C, lengths, 0, top_tokens, top_counts, None)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters   # us per call

    med = lambda v: float(sorted(v)[len(v) // 2])   # noqa: E731
    want_tokens, want_counts = decode_top1(x, lengths, 0)
    results, summary = [], {}
    for beam in (50, 8):
        wsn = int(_lib.call("as_ctc_beam_workspace_bytes", T, B, C, beam))
        ws = torch.empty(wsn, device=dev, dtype=torch.uint8)
        for log_add in (False, True):

            def search():
                _lib.call("as_ctc_beam_search", x, x.stride(1), x.stride(0), T, B, C, 0, lengths, 0, -1, 0.0, beam, C, 50.0,
                          int(log_add), 1, tokens, counts, scores, found, ws, wsn)

            res = ctc_beam_search(x, lengths, beam_size=beam, log_add=log_add)
            if not log_add:
                assert torch.equal(res.counts[:, 0], want_counts) and torch.equal(res.tokens[:, 0], want_tokens)
            differs = int((res.tokens[:, 0] != want_tokens).any(dim=1).sum())
            for _ in range(args.warmup):
                search(), top1()
            torch.cuda.synchronize()
            t_search, t_top1 = [], []
            for _ in range(args.rounds):   # alternating windows
                t_search.append(window(search))
                t_top1.append(window(top1))
            row = dict(workload=f"ctc_beam_search_B{B}_T{T}_C{C}", beam_size=beam, beam_size_token=C, log_add=log_add,
                       workspace_bytes=wsn, utterances_differing_from_best_path=differs,
                       search_us=dict(median=round(med(t_search), 1), min=round(min(t_search), 1), max=round(max(t_search), 1)),
                       decode_top1_us=dict(median=round(med(t_top1), 2), min=round(min(t_top1), 2), max=round(max(t_top1), 2)),
                       search_us_per_frame=round(med(t_search) / T, 2), search_over_decode_top1=round(med(t_search) / med(t_top1), 1),
                       iters=args.iters, rounds=args.rounds)
            print(json.dumps(row), flush=True)
            results.append(row)
            summary[f"beam{beam}_{'log_add' if log_add else 'max'}"] = dict(search_us=row["search_us"]["median"],
                                                                          decode_top1_us=row["decode_top1_us"]["median"])
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"workload": f"CTC beam search of one synthetic batch, B={B}, T={T}, C={C}, beam 50 and 8, both merge rules",
                       "command": "python tools/bench_beam_search.py --out FILE", "device": torch.cuda.get_device_name(0),
                       "timing": "device events around `iters` back-to-back calls per window, alternating windows",
                       "timings": results, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
