#!/usr/bin/env python
"""Cost of evaluating the DeepSpeech2 recogniser on the engine: is validation bound by the model or by the metric?

The thesis recogniser (2 planes x 500 features -> adapter 80, 4 residual blocks, 2 GRU layers of 64, 45 classes) on one batch of
the seeded synthetic data set, B=32 utterances of T=200 frames (targets of about 50 labels):

  (i)   the eval-mode forward (no grad);
  (ii)  EditDistance on the device path (as_decode_top1 + as_edit_distance, two sums, one small copy to the host);
  (iii) the same metric through the host path (the whole emission tensor copied to the host, decoded per utterance and the
        Levenshtein table filled cell by cell in Python) -- the yardstick: what every validation batch paid before;
  (iv)  as_align_counts alone on the decoded batch (the substitution-matrix counts).

(ii) - (iv) run on two sets of emissions: the untrained model's own softmax, and "trained-like" emissions (the per-frame targets
one-hot, 25 % of the frames turned to blank, plus noise: an edit distance near 0.4), whose decoded length is near the targets'.
(ii) and (iii) must return the same float.  Host-clocked around a device synchronise, since (ii) and (iii) end on the host.

    python tools/bench_recognizer_eval.py [--iters N] [--warmup W] [--rounds R] [--out profiles/recognizer_eval_bench.json]

Per-kernel splits: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_recognizer_eval.py --rounds 1` and read DIR's
kernel_stats.csv (the kernels are re_argmax_kernel, re_collapse_kernel, re_edit_distance_kernel, re_align_kernel)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

THESIS = dict(in_channels=2, num_residual_layers=4, num_rnn_layers=2, rnn_hidden_size=64, num_features=500, adapter_out_features=80,
              dropout=0.1, num_classes=45)


def _time(fn, iters, warmup, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    out.sort()
    return dict(ms_median=round(out[len(out) // 2], 4), ms_min=round(out[0], 4), ms_max=round(out[-1], 4), iters=iters, rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from artspeech_amd.phoneme_recognition import Feature, TrainableDeepSpeech2, align_counts
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance, make_pred_and_target_sentences, word_error_rate
    from train_phoneme_recognition import Criterion, build_vocabulary

    dev = torch.device("cuda", 0)
    B, T = 32, 200
    vocabulary = build_vocabulary(None, Criterion.CTC)
    ds = SyntheticPhonemeRecognitionDataset(B, vocabulary, min_len=T, max_len=T, seed=0)
    batch = collate_fn([ds[i] for i in range(B)], [Feature.VOCAL_TRACT])
    x = batch["vocal_tract"].to(dev)
    il, tl = batch["vocal_tract_length"], batch["ctc_target_length"]
    targets = batch["ctc_target"].to(dev)
    torch.manual_seed(0)
    model = TrainableDeepSpeech2(**THESIS).to(dev).eval()
    decoder = GreedyCTCDecoder(list(vocabulary), blank_token="<blank>")
    metric = EditDistance(decoder)

    def forward():
        with torch.no_grad():
            return model(x)

    g = torch.Generator().manual_seed(1)
    frames = batch["articulatory_target"]
    hot = torch.where(torch.rand(B, T, generator=g) < 0.25, torch.zeros_like(frames), frames)
    trained_like = torch.softmax(6.0 * torch.nn.functional.one_hot(hot, len(vocabulary)).float()
                                 + torch.randn(B, T, len(vocabulary), generator=g), -1).to(dev)
    res = [dict(workload=f"eval_forward_B{B}_T{T}", **_time(forward, args.iters, args.warmup, args.rounds))]
    forward_ms = res[0]["ms_median"]
    summary = {}
    for tag, em in (("model", model.get_normalized_outputs(forward())), ("trained_like", trained_like)):
        tokens, counts = decoder.decode_device(em, il)
        host = lambda: word_error_rate(*make_pred_and_target_sentences(decoder, em, targets, il, tl))   # noqa: E731
        value_dev, value_host = metric(em, targets, il, tl), host()
        assert value_dev == value_host, (tag, value_dev, value_host)
        r_dev = _time(lambda: metric(em, targets, il, tl), args.iters, args.warmup, args.rounds)
        r_host = _time(host, max(1, args.iters // 5), 1, args.rounds)
        r_align = _time(lambda: align_counts(tokens, counts, targets, tl, len(vocabulary)), args.iters, args.warmup, args.rounds)
        extra = dict(emissions=tag, edit_distance=value_dev, mean_decoded_tokens=round(float(counts.float().mean()), 1),
                     mean_target_tokens=round(float(tl.float().mean()), 1))
        res += [dict(workload=f"edit_distance_device_B{B}_T{T}", **extra, **r_dev),
                dict(workload=f"edit_distance_host_B{B}_T{T}", **extra, **r_host),
                dict(workload=f"align_counts_B{B}_T{T}", **extra, **r_align)]
        summary[tag] = dict(host_over_device=round(r_host["ms_median"] / r_dev["ms_median"], 1),
                            device_metric_over_forward=round(r_dev["ms_median"] / forward_ms, 3),
                            device_metric_below_forward=r_dev["ms_median"] < forward_ms)
    for r in res:
        print(json.dumps(r), flush=True)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"workload": f"evaluating the thesis DeepSpeech2 recogniser on one synthetic batch, B={B}, T={T}, C={len(vocabulary)}",
                       "command": "python tools/bench_recognizer_eval.py --out FILE", "device": torch.cuda.get_device_name(0),
                       "timings_ms": res, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
