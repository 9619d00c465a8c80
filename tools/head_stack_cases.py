"""Fixed seeded cases through the articulator-head stack (as_head_fwd + as_head_bwd) and through the models that sit on it,
in both matrix arithmetics: one line per case, mode and output buffer with the buffer's SHA-256.  Two commits launch the same
head kernels on the same operands when their digest files are equal and, under
`rocprofv3 --kernel-trace --output-format csv -- python tools/head_stack_cases.py --overlap 0`, their kernel sequences are
(with the side streams on, the order of dispatches is not total: compare the multiset).
usage: python tools/head_stack_cases.py [--overlap 0|1|both] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, N, rows) at A = 3 heads.  Routes (split arithmetic / exact fp32 where they differ):
#   layer 1   planes: H % 32 == 0 in the split arithmetic; fp32 fused: H % 16 == 0 otherwise; general: any other H
#   output    lin_out: 4 <= 2N <= 128; lin plain: 128 < 2N <= 256; general: 2N < 4
#   dx3       fused: 2N % 4 == 0; general otherwise
#   dx1       split slabs: H <= 256, H % 4 == 0, split arithmetic; general: H = 300, H % 4 != 0, or fp32
#   dW        multi: rows % 32 == 0 and rows >= 512; single otherwise
HEAD_CASES = [
    (128, 50, 512),   # l1 planes / fp32 fused; lin_out; dx3 fused; dx1 slabs / general; dW multi
    (128, 50, 37),    # the same layers, dW single; 37 rows: one ragged 32-row tile + a 5-row tail
    (128, 64, 37),    # lin_out at its full 128 columns
    (128, 70, 37),    # output layer: lin plain (O = 140); dx3 fused
    (128, 33, 512),   # lin_out; dx3 general (O = 66)
    (128, 1, 512),    # output layer general (O = 2); dx3 general
    (128, 3, 37),     # lin_out (O = 6); dx3 general
    (64, 33, 512),    # l1 planes / fp32 fused at K = 64; dx1 slabs / general
    (64, 1, 37),
    (50, 3, 37),      # l1 general (H % 16 != 0); dx1 general (H % 4 != 0)
    (50, 64, 512),
    (7, 1, 37),       # every layer-1 route general, output general
    (7, 70, 512),
    (300, 70, 512),   # l1 general (300 % 16 = 12); dx1 general (H > 256); lin plain
    (300, 50, 37),
]
# (H, N, rows) at A = 11 heads: 48 x 11 = 528 whole 64-row tiles, from 512 on the 64-row loops of lin_s6_kernel run (rows and
# shapes of tests/test_gpu_head_tiles.py); the cases above stay below that and run its 32-row loops only
WIDE_HEAD_CASES = [(128, 50, 3021), (96, 40, 3021)]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def head_case(torch, _lib, dev, H, N, rows, A=3):
    L = _lib.lib()
    dims = _lib.Dims(1, A, 1, H, N, 1)
    lay = _lib.layout(dims)
    g = torch.Generator().manual_seed(1000 * H + 10 * N + rows)
    flat = torch.randn(lay.total, generator=g) * 0.08
    for name in ("ln1_g", "ln2_g", "ln3_g"):          # LayerNorm gains around one
        off = int(getattr(lay, name))
        n = A * (H if name == "ln1_g" else 256)
        flat[off:off + n] = 1.0 + 0.3 * torch.randn(n, generator=g)
    x = torch.randn(rows, H, generator=g)
    dsig = torch.randn(rows, A, 2, N, generator=g) * 1e-3
    flat_d, x_d, dsig_d = flat.to(dev), x.to(dev), dsig.to(dev)
    out = torch.full((rows, A, 2, N), float("nan"), device=dev)
    ws = torch.full((L.as_head_workspace_floats(C.byref(dims), rows),), float("nan"), device=dev)
    _lib.check(L.as_head_fwd(C.byref(dims), C.byref(lay), _lib.ptr(flat_d), _lib.ptr(x_d), rows, _lib.ptr(out), _lib.ptr(ws), 1, _lib.stream_ptr()))
    G = torch.zeros_like(flat_d)
    dx = torch.full((rows, H), float("nan"), device=dev)
    _lib.check(L.as_head_bwd(C.byref(dims), C.byref(lay), _lib.ptr(flat_d), _lib.ptr(out), _lib.ptr(dsig_d), rows, _lib.ptr(dx), _lib.ptr(G),
                             _lib.ptr(ws), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return {"out": out, "dx": dx, "grad": G}


def batch(torch, dev, V, A, N, B, T, ragged, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.tensor(sorted((max(1, T - (b * T * 3) // (4 * B)) for b in range(B)), reverse=True) if ragged else [T] * B, dtype=torch.int32)
    tokens = torch.randint(1, V, (B, T), generator=g)
    tgt = torch.rand(B, T, A, 2, N, generator=g)
    for b, l in enumerate(lengths.tolist()):
        tokens[b, l:] = 0
        tgt[b, l:] = 0
    return tokens.to(dev), lengths, tgt.to(dev)


def model_case(torch, dev, cls, H, N, B, T, ragged, dropout, seed):
    """The drop-in module: forward, masked Euclidean criterion, backward."""
    from artspeech_amd.phoneme_to_articulation.metrics import masked_euclidean_loss
    torch.manual_seed(seed)
    model = cls(45, 3, 64, H, N, dropout=dropout).to(dev)
    model.train()
    tokens, lengths, tgt = batch(torch, dev, 45, 3, N, B, T, ragged, seed)
    torch.manual_seed(seed + 1)      # the dropout seed is drawn from torch's CPU generator
    out = model(tokens, lengths)
    loss = masked_euclidean_loss(out, tgt, lengths)
    loss.backward()
    torch.cuda.synchronize()
    return {"contours": out, "loss": loss, "grad": model.flat.grad}


def engine_case(torch, dev, H, N, B, T, pipeline, seed):
    """engine.TrainStep: the criterion rides in the forward (fused into the output layer, or the separate kernel when that
    declines: N = 70); pipeline: layer 2's weight gradient deferred to as_artspeech_dw2 in the next step."""
    from artspeech_amd.engine import TrainStep
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech
    torch.manual_seed(seed)
    model = ArtSpeech(45, 3, 64, H, N).to(dev)
    tokens, lengths, tgt = batch(torch, dev, 45, 3, N, B, T, True, seed)
    step = TrainStep(model, B, T, pipeline=pipeline)
    scale = 1.0 / (float(lengths.sum()) * 3 * N)
    res = {}
    for i in range(2):
        step.step(tokens, lengths.to(dev), tgt, scale)
        torch.cuda.synchronize()
        res[f"step{i}.contours"], res[f"step{i}.loss"] = step.out.clone(), step.loss.clone()
    step.flush()
    torch.cuda.synchronize()
    res["grad"], res["params"] = step.grads, model.flat.data
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--overlap", choices=("0", "1", "both"), default="both", help="side streams of the model-level cases (as_set_overlap)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech, SimpleArtSpeech
    dev = torch.device("cuda:0")
    L = _lib.lib()
    keep = L.as_get_matrix_arith()
    out = open(args.out, "w") if args.out else sys.stdout

    def emit(name, mode, bufs):
        for k, t in bufs.items():
            print(f"{name} arith={mode} {k}={sha(t)}", file=out, flush=True)

    for mode in (1, 0):
        L.as_set_matrix_arith(mode)
        for H, N, rows in HEAD_CASES:
            emit(f"head H={H} N={N} rows={rows}", mode, head_case(torch, _lib, dev, H, N, rows))
        for H, N, rows in WIDE_HEAD_CASES:
            emit(f"head A=11 H={H} N={N} rows={rows}", mode, head_case(torch, _lib, dev, H, N, rows, A=11))
        for ov in ((0, 1) if args.overlap == "both" else (int(args.overlap),)):
            L.as_set_overlap(ov)
            for H in (128, 64):     # H = 128: the trunk's weight gradient rides in the multi launch (2H = 256); H = 64: it does not
                for B, T, ragged in ((4, 128, False), (2, 9, True)):     # 512 rows: dW multi; 18 rows: single
                    emit(f"ArtSpeech H={H} {B}x{T} overlap={ov}", mode, model_case(torch, dev, ArtSpeech, H, 50, B, T, ragged, 0.0, 11))
            emit(f"ArtSpeech dropout H=128 4x128 overlap={ov}", mode, model_case(torch, dev, ArtSpeech, 128, 50, 4, 128, True, 0.3, 12))
            emit(f"engine defer_dw2 H=128 4x128 overlap={ov}", mode, engine_case(torch, dev, 128, 50, 4, 128, True, 13))
            emit(f"engine separate criterion N=70 H=128 4x128 overlap={ov}", mode, engine_case(torch, dev, 128, 70, 4, 128, False, 14))
            # 808 frames: 64-row tiles, a full and an 8-row 32-row tile per head; the fused criterion at its widest (a point per
            # lane) and at its narrowest (4 outputs)
            for N in (64, 2):
                emit(f"engine fused criterion N={N} H=128 8x101 overlap={ov}", mode, engine_case(torch, dev, 128, N, 8, 101, False, 16))
        L.as_set_overlap(1)
        for p in (0.0, 0.3):
            emit(f"SimpleArtSpeech dropout={p} 4x128", mode, model_case(torch, dev, SimpleArtSpeech, 128, 50, 4, 128, False, p, 15))
    L.as_set_matrix_arith(keep)


if __name__ == "__main__":
    main()
