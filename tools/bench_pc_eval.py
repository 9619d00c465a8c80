"""The evaluation of the principal-components method at the thesis shape (10 articulators, N = 50, hidden 50, 35 components): the
device path (as_pc_shapes_eval + as_pc_eval_accumulate) against the same work written with what the engine offered before them --
the per-articulator Normalize.inverse loop, mean_p2cp and torch.cat, and torch.cov of the concatenated latents at the end -- both on
the same GPU, alternating in one process:

  frames     per batch of 64 autoencoder frames: denormalise + MeanP2CPDistance in mm + statistics of errors and latents
  sentences  per batch of B = 32 sentences padded to T = 200: denormalise, inject the upper incisor, errors of the valid frames
  split      a whole split of 32768 frames in batches of 64, through the aggregated table (mean / std / median / min / max) and
             the latent covariance on the host

The inputs of a batch (reconstructions, targets, latents) are made once and reused: the autoencoder itself is the same on both
sides and is not timed.  A time is a host clock around calls that end in a device synchronise; medians over the rounds, after a
warm-up of every shape.  The outputs of the two sides are compared at the sizes that are timed.  Writes
profiles/pc_eval_bench.json.
usage: python tools/bench_pc_eval.py [--iters N] [--warmup W] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd.phoneme_to_articulation.metrics import MeanP2CPDistance  # noqa: E402
from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import (PCEvalState, denorm_tables, median_rows,  # noqa: E402
                                                                                   pc_shapes_eval)
from artspeech_amd.phoneme_to_articulation.transforms import Normalize  # noqa: E402
from artspeech_amd.settings import DATASET_CONFIG  # noqa: E402

ARTS = ["arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate-midline", "thyroid-cartilage",
        "tongue", "upper-lip", "vocal-folds"]
A, N, L = len(ARTS), 50, 35
FRAMES, BATCH, B, T = 32768, 64, 32, 200
REF_IDX = sorted(ARTS + ["upper-incisor"]).index("upper-incisor")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pc_eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pc_eval needs an MI355X: there is no CPU path and no CPU timing stands in for it")
    dev = torch.device("cuda:0")
    cfg = DATASET_CONFIG["artspeech2"]
    to_mm = cfg.PIXEL_SPACING * cfg.RES
    g = torch.Generator().manual_seed(0)
    normalize = {a: Normalize(torch.rand(2, N, generator=g) * 0.5, 0.1 + 0.2 * torch.rand(2, N, generator=g)) for a in ARTS}
    mean, std = denorm_tables(normalize, ARTS, dev)
    p2cp_fn = MeanP2CPDistance(reduction="none")

    # ---- frames: one batch of the autoencoder's evaluation
    recon = torch.rand(BATCH, A, 2 * N, generator=g).to(dev)
    inputs = torch.rand(BATCH, A, 2 * N, generator=g).to(dev)
    latents = torch.randn(BATCH, L, generator=g).mul(0.3).to(dev)

    def frames_device(state):
        _, _, p2cp = pc_shapes_eval(recon, inputs, mean, std, to_mm=to_mm, pred=False, tgt=False)
        state.update(p2cp_mm=p2cp, latents=latents)
        return p2cp

    def frames_stock(acc):
        r = recon.clone().reshape(BATCH, A, 2, N)
        t = inputs.clone().reshape(BATCH, A, 2, N)
        for i, a in enumerate(ARTS):
            r[:, i] = normalize[a].inverse(r[:, i])
            t[:, i] = normalize[a].inverse(t[:, i])
        p2cp = p2cp_fn(r.permute(0, 1, 3, 2), t.permute(0, 1, 3, 2)) * to_mm
        acc["p2cp"] = torch.cat([acc["p2cp"], p2cp])
        acc["latents"] = torch.cat([acc["latents"], latents])
        return p2cp

    def fresh():
        return {"p2cp": torch.zeros(0, A, device=dev), "latents": torch.zeros(0, L, device=dev)}

    # ---- sentences: one batch of the method's evaluation
    lengths = torch.linspace(T, T // 4, B).long().tolist()
    shapes = torch.rand(B, T, A, 2 * N, generator=g).to(dev)
    targets = torch.rand(B, T, A, 2, N, generator=g).to(dev)
    reference = torch.rand(B, T, 1, 2, N, generator=g).to(dev)

    def sentences_device(state):
        pred, tgt, p2cp = pc_shapes_eval(shapes, targets, mean, std, to_mm=to_mm, lengths=lengths, reference=reference, ref_idx=REF_IDX)
        state.update(p2cp_mm=p2cp, lengths=lengths)
        return pred, tgt, p2cp

    def sentences_stock(acc):
        pred = shapes.clone().reshape(B, T, A, 2, N)
        tgt = targets.clone()
        for i, a in enumerate(ARTS):
            pred[..., i, :, :] = normalize[a].inverse(pred[..., i, :, :])
            tgt[..., i, :, :] = normalize[a].inverse(tgt[..., i, :, :])
        p2cp = p2cp_fn(pred.transpose(-1, -2), tgt.transpose(-1, -2)) * to_mm
        acc["p2cp"] = torch.cat([acc["p2cp"]] + [p2cp[i, :n] for i, n in enumerate(lengths)])
        pred = torch.cat([pred[:, :, :REF_IDX], reference, pred[:, :, REF_IDX:]], dim=2)
        tgt = torch.cat([tgt[:, :, :REF_IDX], reference, tgt[:, :, REF_IDX:]], dim=2)
        return pred, tgt, p2cp

    # ---- the whole split
    n_batches = FRAMES // BATCH

    def split_device():
        state = PCEvalState(dev, A, L)
        kept = []
        for _ in range(n_batches):
            kept.append(frames_device(state))
        errors = torch.cat(kept)
        s = state.error_stats()
        agg = torch.stack([s["mean"], s["std"], median_rows(errors), s["min"], s["max"]]).cpu().numpy()
        return agg, state.covariance().cpu().numpy()

    def split_stock():
        acc = fresh()
        for _ in range(n_batches):
            frames_stock(acc)
        cov = torch.cov(acc["latents"].T).cpu().numpy()
        e = acc["p2cp"].cpu().double()
        agg = torch.stack([e.mean(0), e.std(0), e.median(0).values, e.min(0).values, e.max(0).values]).numpy()
        return agg, cov

    result = {"shape": {"articulators": A, "n_samples": N, "latent_size": L, "frames_batch": BATCH, "B": B, "T": T,
                        "valid_sentence_frames": int(sum(lengths)), "split_frames": FRAMES},
              "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds,
              "timing": "host clock around `iters` calls ending in a device synchronise; median / min / max over the rounds; the "
                        "two sides alternate in every round"}

    # outputs of the two sides at the timed sizes
    d_p2cp, s_p2cp = frames_device(PCEvalState(dev, A, L)), frames_stock(fresh())
    d_pred, d_tgt, d_sp2cp = sentences_device(PCEvalState(dev, A))
    s_pred, s_tgt, s_sp2cp = sentences_stock(fresh())
    valid = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(dev)
    d_agg, d_cov = split_device()
    s_agg, s_cov = split_stock()
    result["agreement"] = {
        "frames_p2cp_mm_max_rel": float(((d_p2cp - s_p2cp).abs() / s_p2cp).max()),
        "sentences_p2cp_mm_max_rel_valid": float(((d_sp2cp - s_sp2cp).abs() / s_sp2cp)[valid].max()),
        "sentences_contours_bit_equal_on_valid_frames": bool(torch.equal(d_pred[valid], s_pred[valid])
                                                             and torch.equal(d_tgt[valid], s_tgt[valid])),
        "split_agg_max_rel": float(np.abs(d_agg - s_agg).max() / np.abs(s_agg).max()),
        "split_cov_max_rel": float(np.abs(d_cov - s_cov).max() / np.abs(s_cov).max()),
    }
    print(json.dumps(result["agreement"]), flush=True)

    state_f, state_s = PCEvalState(dev, A, L), PCEvalState(dev, A)
    arms = {
        "frames": {"device": lambda: frames_device(state_f), "stock": None},
        "sentences": {"device": lambda: sentences_device(state_s), "stock": None},
    }
    # the stock side's concatenation grows with the split: it is timed at the split's mid-point (16384 rows already gathered)
    half = {"p2cp": torch.rand(FRAMES // 2, A, device=dev), "latents": torch.rand(FRAMES // 2, L, device=dev)}
    arms["frames"]["stock"] = lambda: frames_stock(dict(half))
    arms["sentences"]["stock"] = lambda: sentences_stock(dict(half))
    for name, sides in arms.items():
        times = {side: [] for side in sides}
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        for _ in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(fn, args.iters))
        result[name + "_ms_per_batch"] = {side: stats(ts) for side, ts in times.items()}
        result[name + "_ms_per_batch"]["stock_over_device"] = round(
            result[name + "_ms_per_batch"]["stock"]["median"] / result[name + "_ms_per_batch"]["device"]["median"], 2)
        print(json.dumps({name: result[name + "_ms_per_batch"]}), flush=True)
    times = {"device": [], "stock": []}
    for _ in range(max(3, args.rounds)):
        times["device"].append(timed(split_device, 1))
        times["stock"].append(timed(split_stock, 1))
    result["split_ms"] = {side: stats(ts) for side, ts in times.items()}
    result["split_ms"]["stock_over_device"] = round(result["split_ms"]["stock"]["median"] / result["split_ms"]["device"]["median"], 2)
    print(json.dumps({"split": result["split_ms"]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
