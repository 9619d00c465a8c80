"""The phoneme-wise mean contour at the thesis shape (10 articulators, N = 50, a 45-token vocabulary, a segmented synthetic train set
of about 50 k frames, batches of B = 32 utterances padded to T = 200) for the per-token sample fractions 0.1 (the reference's) and
1.0: the time of fit() (upload excluded: the data set is resident), of the unweighted and the weighted forward per batch (device
events around single calls after a warm-up, median / min / max over the repeats), the weighted forward's bank traffic -- each
present token's rows read once (what any method must move) and as the kernel streams them (once per tile of 16 queries of a
256-frame chunk) -- over its time, and the same weighted forward written with stock PyTorch ops on the same device (a per-token loop
of nonzero, softmax and matmul), with the largest difference between the two.  Writes profiles/mean_contour_bench.json.
usage: python tools/bench_mean_contour.py [--frames N] [--repeats R] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation.encoder_decoder.dataset import HBMResidentDataset  # noqa: E402
from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import (  # noqa: E402
    PhonemeWiseMeanContour, SyntheticSegmentedArtSpeechDataset, token_runs)
from train_phoneme_to_articulation import build_vocabulary  # noqa: E402

ARTICULATORS = ["arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate-midline", "thyroid-cartilage",
                "tongue", "upper-lip", "vocal-folds"]


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def stock_weighted(model, tokens, rel, lengths):
    """the weighted forward with stock PyTorch ops: a loop over the tokens, softmax over -|rel_k - rel_q| and a matmul each"""
    B, T = tokens.shape
    D = model.row_elems
    valid = (torch.arange(T, device=tokens.device)[None, :] < lengths[:, None]).view(-1)
    flat, bank = tokens.view(-1), model.bank.view(-1, D)
    out = torch.zeros(B * T, D, device=tokens.device)
    offsets = model._offsets_host
    for v in range(model.vocab_size):
        k0, k1 = int(offsets[v]), int(offsets[v + 1])
        if k1 == k0:
            continue
        q = ((flat == v) & valid).nonzero().squeeze(1)
        if q.numel() == 0:
            continue
        w = torch.softmax(-(model.rel_pos[k0:k1][None, :] - rel[q][:, None]).abs(), dim=1)
        out[q] = w @ bank[k0:k1]
    return out.view(B, T, *model.bank.shape[1:])


def bank_traffic(model, tokens, lengths):
    """(bytes with every present token's rows read once, bytes as the kernel streams them)"""
    rows = np.diff(model._offsets_host)
    B, T = tokens.shape
    valid = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    flat = np.where(valid, tokens, -1).reshape(-1)
    row_bytes = model.row_elems * 4
    once = sum(int(rows[v]) for v in np.unique(flat) if v >= 0) * row_bytes
    streamed = 0
    for c in range(0, len(flat), 256):
        present, counts = np.unique(flat[c:c + 256], return_counts=True)
        streamed += sum(int(rows[v]) * -(-int(n) // 16) for v, n in zip(present, counts) if v >= 0) * row_bytes
    return once, streamed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_contour_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mean_contour needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    vocabulary = build_vocabulary(None)
    sentences = max(1, args.frames // 125)
    train = SyntheticSegmentedArtSpeechDataset(sentences, vocabulary, ARTICULATORS, min_len=50, max_len=200, seed=0)
    resident = HBMResidentDataset(train, dev)
    B, T = 32, 200
    batch = SyntheticSegmentedArtSpeechDataset(B, vocabulary, ARTICULATORS, min_len=60, max_len=T, seed=1)
    items = sorted((batch[i] for i in range(B)), key=lambda item: -len(item[1]))
    lengths = [len(item[1]) for item in items]
    tokens = torch.zeros(B, T, dtype=torch.long)
    for b, item in enumerate(items):
        tokens[b, :lengths[b]] = item[1]
    tokens_dev, lengths_dev = tokens.to(dev), torch.tensor(lengths, dtype=torch.int32, device=dev)
    result = {"shape": {"train_frames": int(resident._tokens.numel()), "articulators": len(ARTICULATORS), "n_samples": 50,
                        "vocabulary": len(vocabulary), "B": B, "T": T, "valid_frames": int(sum(lengths))},
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "frac": {}}
    for frac in (0.1, 1.0):
        model = PhonemeWiseMeanContour()
        fit_ms = timed(lambda: model.fit(resident, frac=frac), 1, max(3, args.repeats // 4))
        model.defer_token_check = True
        unweighted = timed(lambda: model.forward(tokens_dev, lengths_dev), 3, args.repeats)
        weighted = timed(lambda: model.forward(tokens_dev, lengths_dev, weighted=True), 3, args.repeats)
        model.check_tokens()
        rel = token_runs(tokens_dev.view(-1), torch.arange(B) * T, lengths)[2]
        stock = timed(lambda: stock_weighted(model, tokens_dev, rel, lengths_dev), 3, args.repeats)
        got, want = model.forward(tokens_dev, lengths_dev, weighted=True), stock_weighted(model, tokens_dev, rel, lengths_dev)
        model.check_tokens()
        once, streamed = bank_traffic(model, tokens.numpy(), lengths)
        out_bytes = B * T * model.row_elems * 4
        seconds = weighted["median"] * 1e-3
        entry = {"bank_rows": int(model.bank.shape[0]), "fit_ms": fit_ms, "unweighted_forward_ms": unweighted,
                 "weighted_forward_ms": weighted, "stock_pytorch_weighted_forward_ms": stock,
                 "weighted_speedup_vs_stock_pytorch": stock["median"] / weighted["median"],
                 "max_abs_difference_vs_stock_pytorch": float((got - want).abs().max()),
                 "bank_bytes_read_once": once, "bank_bytes_streamed_by_the_kernel": streamed, "output_bytes": out_bytes,
                 "weighted_GBps_of_bytes_read_once": (once + out_bytes) / seconds / 1e9,
                 "weighted_GBps_of_bytes_streamed": (streamed + out_bytes) / seconds / 1e9,
                 "weighted_GFLOPs_issued": 2.0 * streamed / 4 * 16 / seconds / 1e9}
        result["frac"][str(frac)] = entry
        print(json.dumps({frac: entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
