#!/usr/bin/env python
"""Cost of training the DeepSpeech2 recogniser (train_phoneme_recognition.py) on the engine, against stock PyTorch on the same GPU:

  (a) the thesis recogniser (2 planes x 500 features -> adapter 80, 4 residual blocks, 2 GRU layers of 64, dropout 0.1, 45 classes)
      at B=4 (the thesis batch) and at B=32, both T=200: the training step (train-mode forward, CTC on the logits with the fused
      log-softmax, backward, torch.optim.Adam) and the no-grad forward;
  (b) the same step in stock PyTorch-ROCm autograd: a torch.nn restatement of the model (tests/recognizer_fp64.py in float32)
      with log_softmax + nn.CTCLoss;
  (c) the CTC kernel alone (loss + gradient) at B=32, T=200, C=45 with targets of 60 labels, and at B=1, T=2100, L=1000;
  (d) as_conv3x3_c32_wgrad alone at B=32, T=200, D=80 (its FLOPs over the 157 TF fp32 matrix peak).

    python tools/bench_recognizer_training.py [--iters N] [--warmup W] [--rounds R] [--out FILE.json] [--only step]

Prints one JSON line per workload (median ms over R rounds of N timed iterations, device-synchronised).  Per-kernel splits:
run `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_recognizer_training.py --only step --rounds 1` and read DIR's
kernel_stats.csv.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

THESIS = dict(in_channels=2, num_residual_layers=4, num_rnn_layers=2, rnn_hidden_size=64, num_features=500, adapter_out_features=80,
              dropout=0.1, num_classes=45)


def _time(fn, iters, warmup, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    out.sort()
    return dict(ms_median=round(out[len(out) // 2], 4), ms_min=round(out[0], 4), ms_max=round(out[-1], 4), iters=iters, rounds=rounds)


def _batch(B, T, dev, C=45, L=40):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 2, 500, T, generator=g).to(dev)
    tg = torch.randint(2, C, (B, L), generator=g).to(dev)
    return x, tg, torch.full((B,), T, dtype=torch.long), torch.full((B,), L, dtype=torch.long)


def step_workloads(dev, B, T, args, stock=True):
    from artspeech_amd.phoneme_recognition import TrainableDeepSpeech2
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    torch.manual_seed(0)
    m = TrainableDeepSpeech2(**THESIS).to(dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-6)
    x, tg, il, tl = _batch(B, T, dev)

    def step():
        opt.zero_grad()
        out = m(x)
        ctc_loss(out.permute(1, 0, 2), tg, il, tl, zero_infinity=True, logits=True).backward()
        opt.step()

    def fwd():
        with torch.no_grad():
            m(x)
    res = [dict(workload=f"engine_train_step_B{B}_T{T}", **_time(step, args.iters, args.warmup, args.rounds)),
           dict(workload=f"engine_fwd_nograd_B{B}_T{T}", **_time(fwd, args.iters, args.warmup, args.rounds))]
    if stock:
        from recognizer_fp64 import DeepSpeech2F64
        torch.manual_seed(0)
        ref = DeepSpeech2F64(**THESIS).float().to(dev).train()
        ropt = torch.optim.Adam(ref.parameters(), lr=1e-4, weight_decay=1e-6)
        crit = torch.nn.CTCLoss(zero_infinity=True)
        n, M = len(ref.residual_layers), len(ref.recurrent_layers)

        def rstep():
            ropt.zero_grad()
            # nn.Dropout(0.1) at the reference's sites, as masks drawn by torch
            masks = {k: F.dropout(torch.ones(B, 32, 80, T, device=dev), 0.1) for k in range(2 * n)}
            masks.update({2 * n + j: F.dropout(torch.ones(T, B, 64, device=dev), 0.1) for j in range(M)})
            masks[2 * n + M] = F.dropout(torch.ones(B, T, 64, device=dev), 0.1)
            out, _ = ref(x, None, masks)
            crit(F.log_softmax(out, -1).permute(1, 0, 2), tg, il, tl).backward()
            ropt.step()
        res.append(dict(workload=f"stock_pytorch_train_step_B{B}_T{T}", **_time(rstep, args.iters, args.warmup, args.rounds)))
    return res


def kernel_workloads(dev, args):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    from artspeech_amd.phoneme_recognition.deepspeech2 import _slab
    res = []
    for B, T, L in ((32, 200, 60), (1, 2100, 1000)):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, B, 45, generator=g).to(dev).requires_grad_(True)
        tg = torch.randint(1, 45, (B, L), generator=g).to(dev)
        il, tl = torch.full((B,), T, dtype=torch.long), torch.full((B,), L, dtype=torch.long)
        fn = lambda: ctc_loss(x, tg, il, tl, zero_infinity=True, logits=True).backward()
        res.append(dict(workload=f"ctc_loss_and_grad_B{B}_T{T}_L{L}", **_time(fn, args.iters, args.warmup, args.rounds)))
    B, T, D = 32, 200, 80
    xa, dy = torch.randn(B, T, D, 32, device=dev), torch.randn(B, T, D, 32, device=dev)
    dw, db = torch.empty(9, 32, 32, device=dev), torch.empty(32, device=dev)
    slab, lib = _slab(dev), _lib.lib()
    fn = lambda: _lib.check(lib.as_conv3x3_c32_wgrad(_lib.ptr(xa), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(db), B, T, D, _lib.ptr(slab),
                                                      slab.numel(), _lib.stream_ptr()))
    r = _time(fn, args.iters * 5, args.warmup, args.rounds)
    flops = 2.0 * B * T * D * 9 * 32 * 32
    r["tflops"] = round(flops / (r["ms_median"] * 1e-3) / 1e12, 1)
    r["share_of_157tf_peak"] = round(r["tflops"] / 157.3, 3)
    res.append(dict(workload="conv3x3_c32_wgrad_B32_T200_D80", **r))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["step", "kernels"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = []
    if args.only in (None, "step"):
        for B in (4, 32):
            res += step_workloads(dev, B, 200, args, stock=args.only is None)
    if args.only in (None, "kernels"):
        res += kernel_workloads(dev, args)
    for r in res:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"workload": "thesis DeepSpeech2 recogniser training (2 planes x 500 features -> adapter 80, 4 residual blocks, "
                                   "2 GRU layers of 64, dropout 0.1, 45 classes), T=200",
                       "command": "python tools/bench_recognizer_training.py --out FILE", "device": torch.cuda.get_device_name(0),
                       "timings_ms": res}, f, indent=1)


if __name__ == "__main__":
    main()
