#!/usr/bin/env python
"""Cost of the input gradient through the frozen DeepSpeech2 scorer and of AutoencoderLoss2's recognition term:

  (a) the thesis scorer (2 planes x 500 features -> adapter 80, 4 residual blocks, 2 GRU layers of 64, 45 classes) at B=32,
      T=200: the no-grad forward, the forward that keeps the backward's activations, and its backward (upstream gradient on
      the features), each timed on its own;
  (b) AutoencoderLoss2 forward + backward at tools/bench_pc_training.py's size (B=12, T=200, 10 articulators x 50 points,
      35 components) without a recognizer (beta4 = 0) and with the thesis scorer (beta4 = 1).

    python tools/bench_scorer_grad.py [--iters N] [--warmup W] [--rounds R] [--out FILE.json] [--only scorer|loss]

Prints one JSON line per workload (median ms over R rounds of N timed iterations, device-synchronised) and writes them all
to --out.  Per-kernel splits: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_scorer_grad.py
--only scorer` and read DIR's kernel_stats.csv.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

THESIS = dict(in_channels=2, num_residual_layers=4, num_rnn_layers=2, rnn_hidden_size=64, num_features=500, adapter_out_features=80)


def _scorer(dev):
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    torch.manual_seed(0)
    m = DeepSpeech2(num_classes=45, **THESIS).to(dev).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def scorer_workloads(dev):
    m = _scorer(dev)
    x = torch.rand(32, 2, 500, 200, device=dev)
    v = (torch.rand(32, 200, device=dev) > 0.5).float()
    xg = x.clone().requires_grad_(True)
    gf = torch.randn(32, 200, 64, device=dev)
    state = {}

    def fwd_nograd():
        with torch.no_grad():
            m(x, v, return_features=True)

    def fwd_keep():
        state["out"] = m(xg, v, return_features=True)[1]

    def bwd():
        torch.autograd.grad(state["out"], xg, gf, retain_graph=True)

    def fwd_bwd():
        torch.autograd.grad(m(xg, v, return_features=True)[1], xg, gf)

    fwd_keep()
    return {"scorer_fwd_nograd": fwd_nograd, "scorer_fwd_keep": fwd_keep, "scorer_bwd": bwd, "scorer_fwd_keep_plus_bwd": fwd_bwd}


def loss_workloads(dev, tmp):
    import bench_pc_training as BP
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    torch.manual_seed(0)
    base = BP._loss(dev, tmp)
    rec = AutoencoderLoss2(BP.COMPS, ["LA", "TTCD", "TBCD"], 100, 50, os.path.join(tmp, "enc.pt"), os.path.join(tmp, "dec.pt"), dev,
                           beta4=1.0, recognizer=_scorer(dev))
    lengths, targets, ref, mask = BP._batch(dev)
    voicing = (torch.rand(12, 200, device=dev) > 0.5).float()
    for b, n in enumerate(lengths.tolist()):
        voicing[b, n:] = -1.0
    pcs = (torch.rand(12, 200, 35, device=dev) * 2 - 1).requires_grad_(True)
    return {"autoencoder_loss2_fwd_bwd_beta4_0": lambda: base(pcs, targets, ref, lengths, mask, voicing).backward(),
            "autoencoder_loss2_fwd_bwd_beta4_1": lambda: rec(pcs, targets, ref, lengths, mask, voicing).backward()}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["scorer", "loss"], default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scorer_grad measures on an MI355X"
    dev = torch.device("cuda:0")
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        wl = {}
        if args.only in (None, "scorer"):
            wl.update(scorer_workloads(dev))
        if args.only in (None, "loss"):
            wl.update(loss_workloads(dev, tmp))
        for fn in wl.values():
            for _ in range(args.warmup):
                fn()
        times = {name: [] for name in wl}
        for _ in range(args.rounds):   # workloads interleaved round by round
            for name, fn in wl.items():
                times[name].append(timed(fn, args.iters))
        for name, ts in times.items():
            ts = sorted(ts)
            r = {"workload": name, "ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                 "iters": args.iters, "rounds": args.rounds}
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
