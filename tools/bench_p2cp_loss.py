"""The point-to-closest-point distance as a training criterion at the benchmark batch (B=32, T=200, A=11, N=50: 70 400 tiles of
50 x 50 distances), in a driver-style loop (no per-call allocation on the library's side), HIP-event time per call:

  fused       as_p2cp_masked_fwd_bwd: loss + d loss / d outputs in one pass (full-length utterances: every tile is computed)
  fused_eval  the same without the gradient (dout = NULL)
  fwd         as_p2cp_fwd alone: the tile values, no gradient -- what the criterion costs on top of the metric
  bwd         as_p2cp_bwd alone (du only), the backward of the module path
  stock       the reference's formulation (metrics.py:27-46) in stock torch ops with autograd on the same GPU:
              cdist -> min over both axes -> mean, backward to the outputs

    python3 tools/bench_p2cp_loss.py [iters] [--json path]     (default path: profiles/p2cp_loss_bench.json)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artspeech_amd import _lib  # noqa: E402


def _time(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def main(iters=None, json_path=None, log=print):
    if iters is None:
        iters = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 30
        json_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else os.path.join(ROOT, "profiles", "p2cp_loss_bench.json")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, T, A, N = 32, 200, 11, 50
    tiles = B * T * A
    out = torch.rand(B, T, A, 2, N, device=dev)
    tgt = torch.rand(B, T, A, 2, N, device=dev)
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    scale = 1.0 / (B * T * A)
    st = _lib.stream_ptr()
    loss = torch.empty((), device=dev)
    dout = torch.empty_like(out)
    partial = torch.empty(L.as_p2cp_masked_partials(), device=dev)
    p2cp = torch.empty(B, T, A, device=dev)
    ones = torch.full((B, T, A), scale, device=dev)

    def fused(grad=True):
        _lib.check(L.as_p2cp_masked_fwd_bwd(_lib.ptr(out), _lib.ptr(tgt), T, _lib.ptr(lengths), B, T, A, N, scale, _lib.ptr(loss),
                                            _lib.ptr(dout if grad else None), _lib.ptr(partial), st), "as_p2cp_masked_fwd_bwd")

    def fwd():
        _lib.check(L.as_p2cp_fwd(_lib.ptr(out), 2 * N, 1, N, N, _lib.ptr(tgt), 2 * N, 1, N, N, tiles, _lib.ptr(p2cp), st), "as_p2cp_fwd")

    def bwd():
        _lib.check(L.as_p2cp_bwd(_lib.ptr(out), 2 * N, 1, N, N, _lib.ptr(tgt), 2 * N, 1, N, N, tiles, _lib.ptr(ones), _lib.ptr(dout),
                                 2 * N, 1, N, None, 0, 0, 0, st), "as_p2cp_bwd")

    leaf = out.clone().requires_grad_(True)

    def stock():
        leaf.grad = None
        d = torch.cdist(leaf.transpose(-1, -2), tgt.transpose(-1, -2))
        per_tile = (d.min(dim=-1).values.sum(-1) / N + d.min(dim=-2).values.sum(-1) / N) / 2
        per_tile.mean().backward()

    cases = {"fused": fused, "fused_eval": lambda: fused(False), "fwd": fwd, "bwd": bwd, "stock": stock}
    report = {"shape": {"B": B, "T": T, "A": A, "N": N, "tiles": tiles}, "iters": iters, "device": torch.cuda.get_device_name(0)}
    log(f"--- B={B} T={T} A={A} N={N} ({tiles} tiles), {iters} calls each, HIP events on the launch stream")
    for name, fn in cases.items():
        us = _time(fn, iters)
        report[name] = {"us_per_call": round(us, 2), "tiles_per_s": round(tiles / (us * 1e-6), 0)}
        log(f"{name:12s} {us:10.2f} us")
    fused()
    fwd()
    torch.cuda.synchronize()
    # the fused value against the metric kernel's tile values (same arithmetic per tile), the fused gradient against stock torch's
    report["fused_loss"] = float(loss)
    report["fwd_mean"] = float(p2cp.double().mean())
    report["grad_max_abs_diff_vs_stock"] = float((dout - leaf.grad).abs().max())
    report["grad_max_abs"] = float(dout.abs().max())
    report["fused_over_fwd"] = round(report["fused"]["us_per_call"] / report["fwd"]["us_per_call"], 3)
    report["stock_over_fused"] = round(report["stock"]["us_per_call"] / report["fused"]["us_per_call"], 2)
    assert abs(report["fused_loss"] - report["fwd_mean"]) <= 1e-5 * report["fwd_mean"], (report["fused_loss"], report["fwd_mean"])
    if json_path:
        with open(json_path, "w") as f:
            json.dump(report, f, indent=1)
    return report


if __name__ == "__main__":
    main()
