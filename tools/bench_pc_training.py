#!/usr/bin/env python
"""Step times of the principal-components method's training at thesis sizes, fused multi-articulator MLP kernel against the
per-articulator GEMM path (autoencoder.FUSED_MLP = False), the two arms alternating in one process:

  (a) AutoencoderLoss2 forward + backward: B=12, T=200, 10 articulators, in 100 / hidden 50 (25 in the middle),
      35 components, TVs LA / TTCD / TBCD, frozen encoder and decoder;
  (b) one MultiArticulatorAutoencoder training step on 2048 frames: forward, RegularizedLatentsMSELoss2, backward, Adam;
  (c) one method training step: PrincipalComponentsArtSpeech (GRU) + AutoencoderLoss2 + backward + Adam.

    python tools/bench_pc_training.py [--iters N] [--warmup W] [--rounds R]

Prints one JSON line per (workload, path): median ms over R rounds of N timed iterations (device-synchronised).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ARTS = ["arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate", "thyroid-cartilage",
        "tongue", "upper-lip", "vocal-folds"]
COMPS = dict(zip(ARTS, (2, 3, 2, 4, 3, 4, 2, 8, 4, 3)))   # 35 components


def _loss(dev, tmp):
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder
    torch.save(MultiEncoder(COMPS, 100, 50).state_dict(), os.path.join(tmp, "enc.pt"))
    torch.save(MultiDecoder(COMPS, 100, 50).state_dict(), os.path.join(tmp, "dec.pt"))
    return AutoencoderLoss2(COMPS, ["LA", "TTCD", "TBCD"], 100, 50, os.path.join(tmp, "enc.pt"), os.path.join(tmp, "dec.pt"), dev)


def _batch(dev, B=12, T=200):
    g = torch.Generator().manual_seed(0)
    lengths = torch.linspace(T, T // 4, B).long()
    targets = (torch.rand(B, T, 10, 2, 50, generator=g) * 0.5).to(dev)
    ref = torch.rand(B, T, 1, 2, 50, generator=g).to(dev)
    mask = (torch.rand(B, 3, T, generator=g) > 0.5).long().to(dev)
    return lengths, targets, ref, mask


def workloads(dev, tmp):
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import (MultiArticulatorAutoencoder,
                                                                                   PrincipalComponentsArtSpeech)
    torch.manual_seed(0)
    crit = _loss(dev, tmp)
    lengths, targets, ref, mask = _batch(dev)
    pcs = (torch.rand(12, 200, 35, device=dev) * 2 - 1).requires_grad_(True)

    def loss_step():
        crit(pcs, targets, ref, lengths, mask).backward()

    ae = MultiArticulatorAutoencoder(100, COMPS, hidden_features=50).to(dev)
    ae_crit = RegularizedLatentsMSELoss2(0.1, ae.indices_dict)
    ae_opt = torch.optim.Adam(ae.parameters(), lr=1e-4)
    frames = torch.rand(2048, 10, 100, device=dev)
    weights = torch.rand(2048, device=dev)

    def ae_step():
        ae_opt.zero_grad()
        out, lat = ae(frames)
        ae_crit(out, lat, frames, weights).backward()
        ae_opt.step()

    model = PrincipalComponentsArtSpeech(45, COMPS, embed_dim=64, hidden_size=128, rnn="gru").to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    tokens = torch.randint(1, 45, (12, 200), device=dev)

    def method_step():
        opt.zero_grad()
        out = model(tokens, lengths.tolist())
        crit(out, targets, ref, lengths, mask).backward()
        opt.step()

    return {"autoencoder_loss2_fwd_bwd": loss_step, "autoencoder_train_step_2048": ae_step, "method_train_step_gru": method_step}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pc_training measures on an MI355X"
    from artspeech_amd.phoneme_to_articulation.principal_components.models import autoencoder
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        wl = workloads(dev, tmp)
        for name, fn in wl.items():
            times = {"fused": [], "grouped": []}
            for mode in times:
                autoencoder.FUSED_MLP = mode == "fused"
                for _ in range(args.warmup):
                    fn()
            for _ in range(args.rounds):
                for mode in times:
                    autoencoder.FUSED_MLP = mode == "fused"
                    times[mode].append(timed(fn, args.iters))
            for mode, ts in times.items():
                ts = sorted(ts)
                print(json.dumps({"workload": name, "path": mode, "ms_median": round(ts[len(ts) // 2], 4),
                                  "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4), "iters": args.iters,
                                  "rounds": args.rounds}), flush=True)
        autoencoder.FUSED_MLP = True


if __name__ == "__main__":
    main()
