"""Every entry point that turns a run-time number into a kernel's template argument (as_up_to / as_exactly / as_flag,
csrc/as_common.h), called once on either side of each boundary of its list at the smallest shapes that reach it: seeded inputs,
one line per case with the SHA-256 of each output.  Two commits pick the same kernels when their digest files are equal and, under
`rocprofv3 --kernel-trace --output-format csv -- python tools/dispatch_cases.py`, their kernel-name sequences are (everything
runs on one stream, so the order is total).  A case the library refuses prints its message instead of digests.
usage: python tools/dispatch_cases.py [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = 5                                                              # one full workgroup of four rows and a partial one
WIDTHS = [64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2816]     # either side of each 64 * N boundary of the row kernels
SPLIT_WIDTHS = [1280, 1100]                                           # the 16-byte backward kernel (D % 256 == 0, D > 1024) / the scalar one
KEYS = [32, 33, 64, 65, 128, 129, 192, 193, 224, 225, 256]            # attention: 1, 2, 4, 6, 7, 8 blocks of 32 keys
TARGETS = [62, 63, 64, 126, 127, 128, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024, 2046, 2047]   # edit distance: L_max / 64 + 1 chunks
HIDDEN = [20, 32, 64, 128]                                            # recurrences: plain kernel, then the three register-resident sizes


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition import align
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else sys.stdout
    call = _lib.call

    def rnd(g, *shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    def empty(*shape, dtype=torch.float32):
        return torch.zeros(*shape, device=dev, dtype=dtype)

    def case(name, seed, fn):
        g = torch.Generator().manual_seed(seed)
        try:
            bufs = fn(g)
            torch.cuda.synchronize()
            print(name + " " + " ".join(f"{k}={sha(t)}" for k, t in bufs.items()), file=out, flush=True)
        except RuntimeError as e:
            print(f"{name} refused: {e}", file=out, flush=True)

    # ---- row kernels: LayerNorm forward (affine / plain / block-major residual), backward (masked / unmasked)
    def ln_fwd(D, affine):
        def run(g):
            x, res = rnd(g, ROWS, D), rnd(g, ROWS, D)
            gamma, beta = (rnd(g, D), rnd(g, D)) if affine else (None, None)
            y, xhat, rstd = empty(ROWS, D), empty(ROWS, D), empty(ROWS)
            call("as_layernorm_fwd", x, res, gamma, beta, y, xhat, rstd, ROWS, D, 0)
            return {"y": y, "xhat": xhat, "rstd": rstd}
        return run

    def ln_blockres(D, per):
        def run(g):
            block = D // per
            x, res = rnd(g, 1, ROWS, D), rnd(g, per, ROWS, block)
            xhat, rstd = empty(ROWS, D), empty(ROWS)
            call("as_layernorm_fwd_blockres", x, res, xhat, rstd, 1, ROWS, per, block)
            return {"xhat": xhat, "rstd": rstd}
        return run

    def ln_bwd(D, masked):
        def run(g):
            dy, xhat, rstd = rnd(g, ROWS, D), rnd(g, ROWS, D), rnd(g, ROWS).abs() + 0.5
            relu_src = rnd(g, ROWS, D) if masked else None
            dx = empty(ROWS, D)
            call("as_layernorm_bwd", dy, xhat, rstd, relu_src, dx, ROWS, D)
            return {"dx": dx}
        return run

    for D in WIDTHS + SPLIT_WIDTHS:
        for affine in (True, False):
            case(f"layernorm_fwd D={D} affine={int(affine)}", D, ln_fwd(D, affine))
        # blocks of 64 where D allows (the WHOLE kernel), else the smallest split into more than one block; and blocks of 32
        pers = [D // 64, D // 32] if D % 64 == 0 else [next((p for p in range(2, 50) if D % p == 0), 1)]
        for per in pers:
            case(f"layernorm_fwd_blockres D={D} per={per}", D, ln_blockres(D, per))
        for masked in (True, False):
            case(f"layernorm_bwd D={D} masked={int(masked)}", D, ln_bwd(D, masked))

    # ---- the head stack: as_normalize_fwd over H with its bit image, and the masked backward that reads the bits
    def head(H):
        def run(g):
            A, N = 3, 3
            dims = _lib.Dims(1, A, 1, H, N, 1)
            lay = _lib.layout(dims)
            flat = rnd(g, lay.total, scale=0.08)
            x, dsig = rnd(g, ROWS, H), rnd(g, ROWS, A, 2, N, scale=1e-3)
            y = empty(ROWS, A, 2, N)
            ws = empty(call("as_head_workspace_floats", dims, ROWS))
            call("as_head_fwd", dims, lay, flat, x, ROWS, y, ws, 1)
            G, dx = torch.zeros_like(flat), empty(ROWS, H)
            call("as_head_bwd", dims, lay, flat, y, dsig, ROWS, dx, G, ws)
            return {"out": y, "dx": dx, "grad": G}
        return run

    for H in (64, 65, 128, 129, 256, 257, 512):
        case(f"head H={H}", H, head(H))

    # ---- softmax over Tk, forward and backward
    def softmax(Tk):
        def run(g):
            Z, Tq = 2, 3
            s, dp = rnd(g, Z, Tq, Tk), rnd(g, Z, Tq, Tk)
            call("as_attn_softmax", s, Z, Tq, Tk, 2, 1, 0.125, None, None)
            call("as_attn_softmax_bwd", s, dp, Z, Tq, Tk, 0.125)
            return {"probs": s, "dscores": dp}
        return run

    for Tk in [w for w in WIDTHS if w <= 1024]:
        case(f"softmax Tk={Tk}", Tk, softmax(Tk))

    # ---- fused attention: forward, dS, and both under a causal mask
    def attention(d, T, causal):
        def run(g):
            heads, Z, Tp = 2, 2, (T + 31) // 32 * 32
            Q, K, V, dctx = (rnd(g, 1, T, d) for _ in range(4))
            ctx, lse, Pt, dSt = empty(1, T, d), empty(Z, T), empty(Z, T, Tp), empty(Z, T, Tp)
            mask = None
            if causal:   # key-major [B][Tk32][T]: -inf where the key comes after the query, zero padding
                mask = empty(1, Tp, T)
                k, q = torch.arange(T, device=dev)[:, None], torch.arange(T, device=dev)[None, :]
                mask[0, :T] = torch.where(k > q, float("-inf"), 0.0)
            call("as_attention_fwd_causal" if causal else "as_attention_fwd", Q, K, V, mask, None, ctx, lse, Pt, 1, 1, heads, T, T, d, d ** -0.5)
            call("as_attention_bwd_ds_causal" if causal else "as_attention_bwd_ds", V, dctx, ctx, Pt, dSt, 1, 1, heads, T, T, d, d ** -0.5)
            return {"ctx": ctx, "lse": lse, "probs_t": Pt, "ds_t": dSt}
        return run

    for d in (32, 64, 128):
        for T in KEYS:
            for causal in (False, True):
                case(f"attention d={d} T={T} causal={int(causal)}", 1000 * d + T, attention(d, T, causal))

    # ---- edit distance over L_max
    def edit(L):
        def run(g):
            B, P = 5, 9
            pred = torch.randint(0, 4, (B, P), generator=g, dtype=torch.int32).to(dev)
            target = torch.randint(0, 4, (B, L), generator=g, dtype=torch.int32).to(dev)
            pc = torch.tensor([9, 1, 0, 5, 9], dtype=torch.int32, device=dev)
            tc = torch.tensor([L, L // 2, L, 0, 1], dtype=torch.int32, device=dev)
            return {"dist": align.edit_distance(pred, pc, target, tc)}
        return run

    for L in TARGETS:
        case(f"edit_distance L_max={L}", L, edit(L))

    # ---- the recogniser's stem: forward, input gradient, weight gradient over the input planes
    def stem(Cin):
        def run(g):
            B, T, D = 1, 7, 5
            x, w, bias, dy = rnd(g, B, Cin, D, T), rnd(g, 9, 32, Cin), rnd(g, 32), rnd(g, B, T, D, 32)
            strides = (Cin * D * T, D * T, T, 1)
            y = empty(B, T, D, 32)
            call("as_conv3x3_stem", x, *strides, w, bias, None, y, B, T, D, Cin)
            bufs = {"y": y}
            if Cin <= 4:
                dx, dw, db = empty(B, Cin, D, T), empty(9, 32, Cin), empty(32)
                ws = empty(256 * (288 * Cin + 32))
                call("as_conv3x3_stem_bwd", dy, w, dx, *strides, B, T, D, Cin)
                call("as_conv3x3_stem_wgrad", x, *strides, dy, dw, db, B, T, D, Cin, ws, ws.numel())
                bufs.update(dx=dx, dw=dw, dbias=db)
            return bufs
        return run

    for Cin in (1, 2, 3, 4, 5):
        case(f"stem Cin={Cin}", Cin, stem(Cin))

    # ---- recurrences: bidirectional GRU and LSTM with (gates saved, token table) as flags, the GRU's one-directional kernels
    B, T, V = 2, 3, 7
    lengths = torch.tensor([3, 2], dtype=torch.int32, device=dev)

    def bidir(kind, H, train, table):
        def run(g):
            NG = 3 if kind == "gru" else 4
            gi = rnd(g, V if table else B * T, 2, NG * H)
            tokens = torch.randint(0, V, (B, T), generator=g).to(dev) if table else None
            w_hh, b_hh, dy = rnd(g, 2, NG * H, H, scale=0.2), rnd(g, 2, NG * H), rnd(g, B, T, 2 * H)
            y = empty(B, T, 2 * H)
            gates = empty(B, T, 2, NG + 1, H) if train else None
            call(f"as_{kind}_bidir_fwd", gi, tokens, T, w_hh, b_hh, lengths, B, T, H, y, gates)
            bufs = {"y": y}
            if train:
                dgi, dgh = empty(B * T, 2 * NG * H), empty(B * T, 2 * NG * H)
                if kind == "gru":
                    call("as_gru_bidir_bwd", dy, y, gates, w_hh, lengths, B, T, H, dgi, dgh)
                else:
                    call("as_lstm_bidir_bwd", dy, gates, w_hh, lengths, B, T, H, dgi)
                bufs.update(gates=gates, dgi=dgi, dgh=dgh)
            return bufs
        return run

    def unidir(H, train):
        def run(g):
            gi, w_hh, b_hh, dy = rnd(g, B * T, 3 * H), rnd(g, 3 * H, H, scale=0.2), rnd(g, 3 * H), rnd(g, B, T, H)
            y = empty(B, T, H)
            if not train:
                call("as_gru_unidir_fwd", gi, w_hh, b_hh, lengths, B, T, H, y)
                return {"y": y}
            gates, dgi, dgh = empty(B * T, 4 * H), empty(B * T, 3 * H), empty(B * T, 3 * H)
            call("as_gru_unidir_fwd_gates", gi, w_hh, b_hh, lengths, B, T, H, y, gates)
            call("as_gru_unidir_bwd", dy, y, gates, w_hh, lengths, B, T, H, dgi, dgh)
            return {"y": y, "gates": gates, "dgi": dgi, "dgh": dgh}
        return run

    for H in HIDDEN:
        for train in (True, False):
            for kind in ("gru", "lstm"):
                for table in (True, False):
                    case(f"{kind} bidir H={H} train={int(train)} table={int(table)}", H, bidir(kind, H, train, table))
            case(f"gru unidir H={H} train={int(train)}", H, unidir(H, train))


if __name__ == "__main__":
    main()
