"""Direct checks of every C entry point of csrc/rowops.hip at each width its dispatch distinguishes: LayerNorm forward
(NW = 1, 2, 4, 8, 16, 44; affine, affine-free, affine-free with whole 64-float words; grouped parameter sets), its block-major
residual form at narrow rows, LayerNorm backward (MW = 2, 4, 8, 44, the 16-byte kernel and its scalar fallback, the ReLU
mask, dx == dy), the masked softmax and its backward (NW = 1 .. 16), fold / unfold of the LayerNorm affine, the group
reduction and the element-wise / gather helpers.  Every reference is plain float64 numpy of the same formula on the same
fp32 inputs (bit equality where the operation is exact in fp32); every output buffer starts as NaN and carries a NaN guard
row (or tail) behind the region the kernel may write.  tests/test_host.py requires every `extern "C"` name of rowops.hip to
occur in this file (as_adam_step and as_gather_pad_rows are tested elsewhere)."""
import numpy as np
import pytest
import torch

from conftest import WORST, assert_grad_close
from test_gpu_attention import _general_mask, _ragged_kpm

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 1e-5
GRID_CAP = 2048 * 256   # elements one pass of the element-wise kernels' grid covers (ew_grid); beyond it the stride loop runs
CPU = torch.device("cpu")

# widths on both sides of every dispatch boundary (64, 128, 256, 512, 1024) and the two ends (1, 2; 2815, 2816 = 64 * 44)
LN_DS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2815, 2816]
TKS = [1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024]
ROWS = [1, 3, 5, 37, 1031]   # 1, 3, 5: a partial workgroup of 4 rows; 1031: 258 workgroups, the last one partial


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _L():
    from artspeech_amd import _lib
    return _lib, _lib.lib()


def _dev(a, dev):
    """numpy -> device tensor.  The caller keeps the result in a local until the call has run: a temporary handed to
    _lib.ptr() is freed at once, and the next allocation reuses its memory while the kernel is still to read it."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _guarded(buf, n, what):
    """buf[:n] fully written (no NaN), buf[n:] (the guard) still NaN"""
    assert torch.isnan(buf[n:]).all(), f"{what}: guard behind the output written"
    assert not torch.isnan(buf[:n]).any(), f"{what}: NaN left in the output"


def _close(got, ref, rtol, atol, family, what):
    """|got - ref| <= atol + rtol |ref| for every element; keeps the family's worst max|got - ref| / max|ref|"""
    a, b = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    rel = float(err.max()) / max(float(np.abs(b).max()), 1e-30)
    WORST["rowops " + family] = max(WORST.get("rowops " + family, 0.0), rel)
    viol = float((err - (atol + rtol * np.abs(b))).max())
    assert viol <= 0, f"{what}: exceeds {atol:g} + {rtol:g} |ref| by {viol:.3e}; max|got - ref| / max|ref| = {rel:.3e}"
    return rel


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got.cpu().numpy() if torch.is_tensor(got) else got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ in bits, first at flat index {int(bad[0])}"


def _refused(rc, code, what):
    _lib, L = _L()
    assert rc == code, f"{what}: returned {rc}, expected {code}"
    with pytest.raises(RuntimeError, match=what.split(":")[0]):
        _lib.check(rc, what)


# --- a. as_layernorm_fwd ---------------------------------------------------------------------------------------------------
def _param_set(rows, group_rows):
    r = np.arange(rows)
    return r // group_rows if group_rows > 0 else (r % (-group_rows) if group_rows < 0 else np.zeros(rows, np.int64))


def _ln_fwd_inputs(D, rows, group_rows, affine, residual, seed, shift=0.0):
    rng = np.random.RandomState(seed)
    # D <= 2: two unit-scale values that nearly coincide make x - mean a cancellation whose fp32 rounding no implementation
    # avoids (in 1031 random rows stock fp32 torch reaches 0.46 of the bound on xhat and 1.04 of it on y); on a grid of
    # eighths the sum, the mean and x - mean are exact in fp32, and a wrong formula shows all the same
    draw = (lambda: rng.randint(-24, 25, (rows, D)) / 8.0) if D <= 2 else (lambda: rng.randn(rows, D))
    x = (shift + draw()).astype(np.float32)
    res = draw().astype(np.float32) if residual else None
    sets = int(_param_set(rows, group_rows).max()) + 1
    # every parameter set is an independent unit-scale draw: a wrong set index moves every element of y by O(1)
    gamma = (0.5 + rng.rand(sets, D)).astype(np.float32) if affine else None
    beta = rng.randn(sets, D).astype(np.float32) if affine else None
    return x, res, gamma, beta


def _ln_fwd_ref(x, res, gamma, beta, group_rows):
    z = x.astype(np.float64) + (res.astype(np.float64) if res is not None else 0.0)
    mu = z.mean(-1, keepdims=True)
    var = ((z - mu) ** 2).mean(-1, keepdims=True)   # two-pass, as the kernel
    rs = 1.0 / np.sqrt(var + EPS)
    xhat = (z - mu) * rs
    y = xhat
    if gamma is not None:
        s = _param_set(x.shape[0], group_rows)
        y = xhat * gamma.astype(np.float64)[s] + beta.astype(np.float64)[s]
    return y, xhat, rs[:, 0]


def _ln_fwd_run(dev, x, res, gamma, beta, group_rows, want_y, want_xhat, want_rstd):
    _lib, L = _L()
    rows, D = x.shape
    tx, tres, tg, tb = (None if a is None else _dev(a, dev) for a in (x, res, gamma, beta))
    y = _nan(dev, rows + 1, D) if want_y else None
    xhat = _nan(dev, rows + 1, D) if want_xhat else None
    rstd = _nan(dev, rows + 1) if want_rstd else None
    rc = L.as_layernorm_fwd(_lib.ptr(tx), _lib.ptr(tres), _lib.ptr(tg), _lib.ptr(tb), _lib.ptr(y), _lib.ptr(xhat), _lib.ptr(rstd),
                            rows, D, group_rows, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, y, xhat, rstd


_LN_MODES = ("plain", "affine", "grouped", "interleaved")   # no gamma / one set / group_rows = 3 / group_rows = -3
_OUTS = ((True, False), (False, True), (True, True))          # (y, xhat)


@pytest.mark.parametrize("mode", _LN_MODES)
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_fwd_every_width(dev, D, mode):
    """as_layernorm_fwd at every register width, affine-free (whole-word variant at D % 64 == 0) and affine with one
    parameter set, with blocks of 3 rows per set (rows is never a multiple of 3: the last block is short) and with set =
    row % 3; residual, the kept outputs and rstd vary from case to case so that each is on and off at every NW."""
    _lib, L = _L()
    i = LN_DS.index(D) + 5 * _LN_MODES.index(mode)
    group_rows = {"plain": 0, "affine": 0, "grouped": 3, "interleaved": -3}[mode]
    rows = [5, 37, 1031][i % 3] if group_rows else ROWS[i % 5]
    residual, (want_y, want_xhat), want_rstd = bool(i % 2), _OUTS[(i // 2) % 3], bool((i // 3) % 2)
    x, res, gamma, beta = _ln_fwd_inputs(D, rows, group_rows, mode != "plain", residual, seed=1000 * D + i)
    ry, rxhat, rrs = _ln_fwd_ref(x, res, gamma, beta, group_rows)
    rc, y, xhat, rstd = _ln_fwd_run(dev, x, res, gamma, beta, group_rows, want_y, want_xhat, want_rstd)
    _lib.check(rc, "as_layernorm_fwd")
    what = f"as_layernorm_fwd D={D} rows={rows} {mode} residual={residual}"
    if want_y:
        _guarded(y, rows, what + ": y")
        _close(y[:rows].cpu().numpy(), ry, 2e-5, 2e-5, "layernorm_fwd y", what + ": y")
    if want_xhat:
        _guarded(xhat, rows, what + ": xhat")
        _close(xhat[:rows].cpu().numpy(), rxhat, 2e-5, 2e-5, "layernorm_fwd xhat", what + ": xhat")
    if want_rstd:
        _guarded(rstd, rows, what + ": rstd")
        _close(rstd[:rows].cpu().numpy(), rrs, 2e-5, 0.0, "layernorm_fwd rstd", what + ": rstd")


def test_layernorm_fwd_refuses_rows_wider_than_2816(dev):
    x, res, gamma, beta = _ln_fwd_inputs(2817, 3, 0, True, False, seed=1)
    rc, y, xhat, rstd = _ln_fwd_run(dev, x, res, gamma, beta, 0, True, True, True)
    _refused(rc, -2, "as_layernorm_fwd: unsupported row length")
    assert "2817" in _L()[1].as_last_error().decode()
    for t in (y, xhat, rstd):
        assert torch.isnan(t).all()


# The shifted row (mean 100, spread 1) separates a two-pass variance from E[x^2] - mean^2, whose fp32 cancellation
# (1e4 against 1) is worth ~1e-3 of xhat.  Bound = 4 x the error of stock fp32 torch.nn.functional.layer_norm on the CPU
# against the float64 reference on these very inputs (the kernel adds a row in another order than torch):
#   torch fp32: max|xhat - ref| = 1.231e-5, max|rstd - ref| / ref = 1.029e-7   ->   bounds 4.92e-5 (absolute) and 4.12e-7 (relative)
# (the same rows through E[x^2] - mean^2 in fp32: max|xhat - ref| = 2.8e-3)
_SHIFT_XHAT_ATOL, _SHIFT_RSTD_RTOL = 4 * 1.231e-5, 4 * 1.029e-7


def _shifted_inputs():
    return _ln_fwd_inputs(512, 37, 0, False, False, seed=77, shift=100.0)


def test_layernorm_fwd_shifted_rows_need_a_two_pass_variance(dev):
    _lib, L = _L()
    x, res, gamma, beta = _shifted_inputs()
    _, rxhat, rrs = _ln_fwd_ref(x, None, None, None, 0)
    rc, _, xhat, rstd = _ln_fwd_run(dev, x, None, None, None, 0, False, True, True)
    _lib.check(rc, "as_layernorm_fwd")
    _guarded(xhat, 37, "shifted xhat")
    _close(xhat[:37].cpu().numpy(), rxhat, 0.0, _SHIFT_XHAT_ATOL, "layernorm_fwd shifted xhat", "row mean 100: xhat")
    _close(rstd[:37].cpu().numpy(), rrs, _SHIFT_RSTD_RTOL, 0.0, "layernorm_fwd shifted rstd", "row mean 100: rstd")


# --- b. as_layernorm_fwd_blockres at narrow rows ----------------------------------------------------------------------------
def _blockres_inputs(channels, rows, per, block, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(channels, rows, per * block).astype(np.float32), rng.randn(channels * per, rows, block).astype(np.float32)


def _blockres_ref(x, q, per, block):
    channels, rows, D = x.shape
    z = x.astype(np.float64) + q.astype(np.float64).reshape(channels, per, rows, block).transpose(0, 2, 1, 3).reshape(channels, rows, D)
    mu = z.mean(-1, keepdims=True)
    var = ((z - mu) ** 2).mean(-1, keepdims=True)
    return (z - mu) / np.sqrt(var + EPS), 1.0 / np.sqrt(var[..., 0] + EPS)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("per,block", [(3, 20), (2, 64), (5, 128), (10, 32), (7, 96)])
def test_layernorm_fwd_blockres_narrow_rows(dev, per, block, channels):
    """The block-major residual at rows of 60 .. 672 floats (NW = 1, 2, 8, 16): blocks that are whole 64-float words (the
    wave-uniform block index) and blocks that are not (the per-lane one, clamped with the lanes beyond the row)."""
    _lib, L = _L()
    for rows in (3, 5, 258):   # per channel: 3, 5, 9, 15 rows in all are no multiple of 4; 258 and 774 are many workgroups
        x, q = _blockres_inputs(channels, rows, per, block, seed=per * block + rows + channels)
        rxhat, rrs = _blockres_ref(x, q, per, block)
        total, D = channels * rows, per * block
        xhat, rstd = _nan(dev, total + 1, D), _nan(dev, total + 1)
        tx, tq = _dev(x, dev), _dev(q, dev)
        _lib.check(L.as_layernorm_fwd_blockres(_lib.ptr(tx), _lib.ptr(tq), _lib.ptr(xhat), _lib.ptr(rstd), channels,
                                               rows, per, block, _lib.stream_ptr()), "as_layernorm_fwd_blockres")
        torch.cuda.synchronize()
        what = f"as_layernorm_fwd_blockres per={per} block={block} channels={channels} rows={rows}"
        _guarded(xhat, total, what)
        _guarded(rstd, total, what + ": rstd")
        _close(xhat[:total].cpu().numpy(), rxhat.reshape(total, D), 2e-5, 2e-5, "layernorm_fwd_blockres xhat", what)
        _close(rstd[:total].cpu().numpy(), rrs.reshape(total), 2e-5, 0.0, "layernorm_fwd_blockres rstd", what + ": rstd")


# --- c. as_layernorm_bwd ------------------------------------------------------------------------------------------------------
BWD_DS = LN_DS + [1100, 1280, 1536, 2560]   # 1100: MW = 44 without the 16-byte kernel; 1280, 1536, 2560 (and 2816): with it


def _ln_bwd_inputs(D, rows, masked, seed):
    """dy, xhat, rstd (fp32) and the ReLU mask source.  xhat and rstd are the float64 LayerNorm of a unit-scale x rounded to
    fp32 -- except at D <= 2, where a LayerNorm output leaves the formula nothing to compute (the result lives in the D - 2
    dimensions orthogonal to 1 and xhat: exactly 0 at D = 1, 1e-5 of its operands at D = 2, where no fp32 evaluation, stock
    torch included, is within 1e-4 of the maximum); there xhat is a plain random row, which tests the same formula."""
    rng = np.random.RandomState(seed)
    x = rng.randn(rows, D).astype(np.float32)
    _, xhat, rs = _ln_fwd_ref(x, None, None, None, 0)
    if D <= 2:
        xhat = 0.7 * rng.randn(rows, D)
    dy = rng.randn(rows, D).astype(np.float32)
    m = None
    if masked:
        m = rng.randn(rows, D).astype(np.float32)
        f = m.reshape(-1)
        f[0::7], f[1::7] = 0.0, -0.0
        f[2::7], f[3::7] = 1e-40, -1e-40   # denormals: the positive one is > 0 and keeps its element
        f[4::7] = -np.abs(f[4::7])
    return dy, xhat.astype(np.float32), rs.astype(np.float32), m


def _ln_bwd_ref(dy, xhat, rstd, m):
    g, h = dy.astype(np.float64), xhat.astype(np.float64)
    dx = rstd.astype(np.float64)[:, None] * (g - g.mean(-1, keepdims=True) - h * (g * h).mean(-1, keepdims=True))
    return dx if m is None else np.where(m > 0, dx, 0.0)


def _ln_bwd_run(dev, dy, xhat, rstd, m, dy_offset=0, alias=False):
    """-> (rc, dx [rows + 1][D]); dy_offset: dy starts that many floats into its allocation; alias: dx is dy's buffer"""
    _lib, L = _L()
    rows, D = dy.shape
    tdy = _nan(dev, (rows + 1) * D + dy_offset)
    tdy[dy_offset:dy_offset + rows * D] = _dev(dy, dev).reshape(-1)
    tdy_in = tdy[dy_offset:]
    dx = tdy_in if alias else _nan(dev, (rows + 1) * D)
    txh, trs, tm = _dev(xhat, dev), _dev(rstd, dev), (None if m is None else _dev(m, dev))
    rc = L.as_layernorm_bwd(_lib.ptr(tdy_in), _lib.ptr(txh), _lib.ptr(trs), _lib.ptr(tm), _lib.ptr(dx), rows, D, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dx[:(rows + 1) * D].view(rows + 1, D)


def _ln_bwd_check(dx, ref, m, rows, what, family):
    _guarded(dx, rows, what)
    got = dx[:rows].cpu().numpy()
    _close(got, ref, 0.0, 1e-4 * np.abs(ref).max(), family, what)
    if m is not None:
        off = ~(m > 0)
        assert off.any() and (m > 0).any()
        assert (got[off] == 0).all(), f"{what}: a position with !(mask > 0) is not an exact zero"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D", BWD_DS)
def test_layernorm_bwd_every_width(dev, D, masked):
    """as_layernorm_bwd at MW = 2, 4, 8, 44, whole-word and clamped, the 16-byte kernel (D % 256 == 0 above 1024) and the
    ReLU-masked variant at every one of them (MW = 44 at D = 1025 .. 2816 included)."""
    _lib, L = _L()
    i = BWD_DS.index(D) + (2 if masked else 0)
    rows = ROWS[i % 5]
    dy, xhat, rstd, m = _ln_bwd_inputs(D, rows, masked, seed=31 * D + i)
    rc, dx = _ln_bwd_run(dev, dy, xhat, rstd, m)
    _lib.check(rc, "as_layernorm_bwd")
    _ln_bwd_check(dx, _ln_bwd_ref(dy, xhat, rstd, m), m, rows, f"as_layernorm_bwd D={D} rows={rows} masked={masked}",
                  "layernorm_bwd masked" if masked else "layernorm_bwd")


def test_layernorm_bwd_misaligned_dy_takes_the_scalar_kernel(dev):
    """D = 1280 is eligible for the 16-byte kernel; a dy that starts one float into its allocation is not: the call must fall
    back to the scalar kernel (MW = 44, whole words) and meet the same bound as the aligned call."""
    _lib, L = _L()
    D, rows = 1280, 37
    dy, xhat, rstd, _ = _ln_bwd_inputs(D, rows, False, seed=5)
    ref = _ln_bwd_ref(dy, xhat, rstd, None)
    for off in (0, 1):
        rc, dx = _ln_bwd_run(dev, dy, xhat, rstd, None, dy_offset=off)
        _lib.check(rc, "as_layernorm_bwd")
        _ln_bwd_check(dx, ref, None, rows, f"as_layernorm_bwd D=1280, dy offset by {off} float",
                      "layernorm_bwd misaligned dy" if off else "layernorm_bwd")


@pytest.mark.parametrize("D,masked", [(1280, False), (300, False), (64, False), (2816, True), (200, True)])
def test_layernorm_bwd_in_place_is_bit_identical(dev, D, masked):
    """dx == dy (documented): a lane reads all its elements before it writes any -- same bits as out of place"""
    _lib, L = _L()
    rows = 37
    dy, xhat, rstd, m = _ln_bwd_inputs(D, rows, masked, seed=D)
    rc, out = _ln_bwd_run(dev, dy, xhat, rstd, m)
    _lib.check(rc, "as_layernorm_bwd")
    rc, inp = _ln_bwd_run(dev, dy, xhat, rstd, m, alias=True)
    _lib.check(rc, "as_layernorm_bwd")
    _guarded(inp, rows, f"in place D={D}")
    _same_bits(inp[:rows], out[:rows].cpu().numpy(), f"as_layernorm_bwd in place D={D} masked={masked}")


def test_layernorm_bwd_refuses_rows_wider_than_2816(dev):
    dy, xhat, rstd, _ = _ln_bwd_inputs(2817, 3, False, seed=2)
    rc, dx = _ln_bwd_run(dev, dy, xhat, rstd, None)
    _refused(rc, -2, "normalize: unsupported row length")
    assert torch.isnan(dx).all()


# --- d. as_attn_softmax -------------------------------------------------------------------------------------------------------
_SCALE = 0.37


def _softmax_inputs(G, B, heads, Tq, Tk, masks, seed, magnitude=3.0):
    """scores [Z][Tq][Tk] (fp32, |s * scale| ~ magnitude), attn_mask [B][Tq][Tk] / kpm [B][Tk] or None: the builders of
    test_gpu_attention (-inf entries, key 0 visible), drawn on the CPU so that the inputs do not depend on the device"""
    rng = np.random.RandomState(seed)
    s = (rng.randn(G * B * heads, Tq, Tk) * (magnitude / _SCALE)).astype(np.float32)
    am = _general_mask(B, Tq, Tk, CPU, seed).numpy() if masks in ("attn_mask", "both") else None
    kpm = _ragged_kpm(B, Tk, CPU).numpy() if masks in ("kpm", "both") else None
    return s, am, kpm


def _softmax_ref(s, am, kpm, heads, B, scale=_SCALE):
    """float64 softmax(s * scale + attn_mask[b] + kpm[b]) with b = (z / heads) % B; -> (P, the additive mask per z)"""
    Z, Tq, Tk = s.shape
    b = (np.arange(Z) // heads) % B
    add = np.zeros((Z, Tq, Tk))
    if am is not None:
        add = add + am.astype(np.float64)[b]
    if kpm is not None:
        add = add + kpm.astype(np.float64)[b][:, None, :]
    x = s.astype(np.float64) * float(np.float32(scale)) + add
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True), add


def _softmax_run(dev, s, am, kpm, heads, B, scale=_SCALE):
    _lib, L = _L()
    Z, Tq, Tk = s.shape
    buf = _nan(dev, Z * Tq + 1, Tk)
    buf[:Z * Tq] = _dev(s, dev).view(Z * Tq, Tk)
    tam, tk = (None if a is None else _dev(a, dev) for a in (am, kpm))
    rc = L.as_attn_softmax(_lib.ptr(buf), Z, Tq, Tk, heads, B, scale, _lib.ptr(tam), _lib.ptr(tk), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf


_MASKS = ("none", "attn_mask", "kpm", "both")
_GBH = (2, 3, 2)   # G channel groups x B utterances x heads: b = (z / heads) % B wraps across the groups


@pytest.mark.parametrize("Tk", TKS)
def test_attn_softmax_every_key_count(dev, Tk):
    """as_attn_softmax at NW = 1, 2, 4, 8, 16 and both sides of every boundary, Tq = 1, 5, 37, every mask combination; the
    probabilities against float64 and exact zeros where a mask is -inf.  (G, B, heads) = (1, 3, 1) at Tq = 1 and 5 gives 3 and
    15 rows (a partial workgroup); (2, 3, 2) at Tq = 37 gives 444 rows (111 workgroups)."""
    _lib, L = _L()
    for Tq in (1, 5, 37):
        for masks in _MASKS:
            for G, B, heads in ((_GBH,) if Tq == 37 else (_GBH, (1, 3, 1))):
                s, am, kpm = _softmax_inputs(G, B, heads, Tq, Tk, masks, seed=Tk * 41 + Tq)
                ref, add = _softmax_ref(s, am, kpm, heads, B)
                rc, buf = _softmax_run(dev, s, am, kpm, heads, B)
                _lib.check(rc, "as_attn_softmax")
                rows = s.shape[0] * Tq
                what = f"as_attn_softmax Tk={Tk} Tq={Tq} masks={masks} Z={s.shape[0]}"
                _guarded(buf, rows, what)
                got = buf[:rows].cpu().numpy().reshape(ref.shape)
                _close(got, ref, 0.0, 1e-5 * ref.max(), "attn_softmax", what)
                assert (got[np.isneginf(add)] == 0).all(), f"{what}: a masked position is not an exact zero"


# |s * scale| ~ 80: without the subtraction of the row maximum exp overflows (e^89 > FLT_MAX).  Bound = 4 x the error of stock
# fp32 torch.softmax(s * scale + attn_mask + kpm) on the CPU against the float64 reference on these very inputs:
#   torch fp32: max|p - ref| / max|ref| = 1.425e-6   ->   bound 5.70e-6 (of max|ref|)
_BIG_SCORE_TOL = 4 * 1.425e-6


def _big_score_inputs():
    return _softmax_inputs(*_GBH, 5, 300, "both", seed=80, magnitude=80.0)


def test_attn_softmax_large_scores_subtract_the_row_maximum(dev):
    _lib, L = _L()
    s, am, kpm = _big_score_inputs()
    assert np.abs(s * np.float32(_SCALE)).max() > 200
    ref, add = _softmax_ref(s, am, kpm, _GBH[2], _GBH[1])
    rc, buf = _softmax_run(dev, s, am, kpm, _GBH[2], _GBH[1])
    _lib.check(rc, "as_attn_softmax")
    _guarded(buf, 60, "large scores")
    got = buf[:60].cpu().numpy().reshape(ref.shape)
    _close(got, ref, 0.0, _BIG_SCORE_TOL * ref.max(), "attn_softmax large scores", "as_attn_softmax |score| ~ 80")
    assert (got[np.isneginf(add)] == 0).all()


@pytest.mark.parametrize("Tk", [65, 513])
def test_attn_softmax_fully_masked_row_is_nan_there_only(dev, Tk):
    """PyTorch semantics: the one (utterance, query) row whose keys are all -inf gives NaN for every head and channel group,
    every other row is unaffected"""
    _lib, L = _L()
    G, B, heads = _GBH
    Tq, b0, q0 = 5, 1, 3
    s, am, kpm = _softmax_inputs(G, B, heads, Tq, Tk, "both", seed=Tk)
    am[b0, q0, :] = -np.inf
    ref, _ = _softmax_ref(s, am, kpm, heads, B)
    rc, buf = _softmax_run(dev, s, am, kpm, heads, B)
    _lib.check(rc, "as_attn_softmax")
    got = buf[:G * B * heads * Tq].cpu().numpy().reshape(ref.shape)
    expect = np.zeros(ref.shape, bool)
    expect[(np.arange(G * B * heads) // heads) % B == b0, q0, :] = True
    assert expect.sum() == G * heads * Tk and np.array_equal(np.isnan(ref), expect)
    assert np.array_equal(np.isnan(got), expect)
    assert torch.isnan(buf[G * B * heads * Tq:]).all()
    _close(np.nan_to_num(got), np.nan_to_num(ref), 0.0, 1e-5 * np.nanmax(ref), "attn_softmax", f"fully masked row, Tk={Tk}")


def test_attn_softmax_refuses_more_than_1024_keys(dev):
    s, am, kpm = _softmax_inputs(1, 1, 1, 2, 1025, "none", seed=3)
    rc, buf = _softmax_run(dev, s, None, None, 1, 1)
    _refused(rc, -2, "as_attn_softmax: unsupported key count")
    assert "1024" in _L()[1].as_last_error().decode()
    _same_bits(buf[:2], s.reshape(2, 1025), "scores after a refused call")


# --- e. as_attn_softmax_bwd -----------------------------------------------------------------------------------------------------
def _softmax_bwd_inputs(Tq, Tk, masks, seed, gbh=_GBH):
    """P: the float64 reference rounded to fp32 (exact zeros at masked keys); dP: unit scale, and large finite values where
    P == 0 -- they must meet the factor P == 0, not leak into the row sum"""
    G, B, heads = gbh
    s, am, kpm = _softmax_inputs(G, B, heads, Tq, Tk, masks, seed)
    p64, add = _softmax_ref(s, am, kpm, heads, B)
    p = p64.astype(np.float32)
    dp = np.random.RandomState(seed + 1).randn(*p.shape).astype(np.float32)
    dp[np.isneginf(add)] *= 1e6
    return p, dp, np.isneginf(add)


def _softmax_bwd_ref(p, dp, scale=_SCALE):
    P, dP = p.astype(np.float64), dp.astype(np.float64)
    return P * (dP - (P * dP).sum(-1, keepdims=True)) * float(np.float32(scale))


@pytest.mark.parametrize("Tk", TKS)
def test_attn_softmax_bwd_every_key_count(dev, Tk):
    """as_attn_softmax_bwd, in place on dP, at NW = 1 .. 16 and both sides of every boundary"""
    _lib, L = _L()
    for Tq in (1, 5, 37):
        for masks in ("none", "both"):
            for gbh in ((_GBH,) if Tq == 37 else (_GBH, (1, 3, 1))):
                p, dp, masked = _softmax_bwd_inputs(Tq, Tk, masks, seed=Tk * 17 + Tq, gbh=gbh)
                ref = _softmax_bwd_ref(p, dp)
                rows = p.shape[0] * Tq
                buf = _nan(dev, rows + 1, Tk)
                buf[:rows] = _dev(dp, dev).view(rows, Tk)
                tp = _dev(p, dev)
                _lib.check(L.as_attn_softmax_bwd(_lib.ptr(tp), _lib.ptr(buf), p.shape[0], Tq, Tk, _SCALE, _lib.stream_ptr()),
                           "as_attn_softmax_bwd")
                torch.cuda.synchronize()
                what = f"as_attn_softmax_bwd Tk={Tk} Tq={Tq} masks={masks} Z={p.shape[0]}"
                _guarded(buf, rows, what)
                got = buf[:rows].cpu().numpy().reshape(ref.shape)
                _close(got, ref, 0.0, 2e-5 * np.abs(ref).max(), "attn_softmax_bwd", what)
                assert (got[masked] == 0).all(), f"{what}: dS at a masked key is not an exact zero"


def test_attn_softmax_bwd_refuses_more_than_1024_keys(dev):
    _lib, L = _L()
    p, dp = torch.zeros(2, 1025, device=dev), _nan(dev, 2, 1025)
    rc = L.as_attn_softmax_bwd(_lib.ptr(p), _lib.ptr(dp), 1, 2, 1025, 1.0, _lib.stream_ptr())
    torch.cuda.synchronize()
    _refused(rc, -2, "as_attn_softmax_bwd: unsupported key count")
    assert torch.isnan(dp).all()


# --- f. as_fold_ln / as_unfold_ln -----------------------------------------------------------------------------------------------
def _fold_inputs(heads, R, K, seed):
    rng = np.random.RandomState(seed)
    f = lambda *s: rng.randn(*s).astype(np.float32)
    return dict(W=f(heads, R, K), gamma=(0.5 + rng.rand(heads, K)).astype(np.float32), beta=f(heads, K), b=f(heads, R),
                dWf=f(heads, R, K), dbf=f(heads, R))


def _fold_ref(i):
    W, gamma, beta, b, dWf, dbf = (i[k].astype(np.float64) for k in ("W", "gamma", "beta", "b", "dWf", "dbf"))
    return dict(Wf=W * gamma[:, None, :], bf=b + np.einsum("hrk,hk->hr", W, beta),
                dW=dWf * gamma[:, None, :] + dbf[:, :, None] * beta[:, None, :],
                dgamma=np.einsum("hrk,hrk->hk", dWf, W), dbeta=np.einsum("hr,hrk->hk", dbf, W))


# R = 15, 16, 17, 100, 256 around the unfold kernel's 16 row lanes; K = 63, 64, 65, 200, 256, 2816 around its 64 columns
_FOLD = [(1, 1, 1), (3, 15, 63), (3, 16, 64), (3, 17, 65), (1, 100, 200), (11, 256, 256), (1, 17, 2816), (3, 100, 256), (11, 1, 65),
         (1, 256, 1), (3, 5, 2816), (11, 15, 200)]


@pytest.mark.parametrize("heads,R,K", _FOLD)
def test_fold_and_unfold_ln(dev, heads, R, K):
    _lib, L = _L()
    i = _fold_inputs(heads, R, K, seed=heads * 1000 + R * 7 + K)
    ref = _fold_ref(i)
    t = {k: _dev(v, dev) for k, v in i.items()}
    n = heads * R
    Wf, bf = _nan(dev, n + 1, K), _nan(dev, n + 1)
    _lib.check(L.as_fold_ln(_lib.ptr(t["W"]), _lib.ptr(t["gamma"]), _lib.ptr(t["beta"]), _lib.ptr(t["b"]), _lib.ptr(Wf), _lib.ptr(bf),
                            heads, R, K, _lib.stream_ptr()), "as_fold_ln")
    dW, dgamma, dbeta = _nan(dev, n + 1, K), _nan(dev, heads + 1, K), _nan(dev, heads + 1, K)
    _lib.check(L.as_unfold_ln(_lib.ptr(t["dWf"]), _lib.ptr(t["dbf"]), _lib.ptr(t["W"]), _lib.ptr(t["gamma"]), _lib.ptr(t["beta"]),
                              _lib.ptr(dW), _lib.ptr(dgamma), _lib.ptr(dbeta), heads, R, K, _lib.stream_ptr()), "as_unfold_ln")
    torch.cuda.synchronize()
    what = f"heads={heads} R={R} K={K}"
    for name, buf, rows in (("Wf", Wf, n), ("bf", bf, n), ("dW", dW, n), ("dgamma", dgamma, heads), ("dbeta", dbeta, heads)):
        _guarded(buf, rows, f"{name} {what}")
        got = buf[:rows].cpu().numpy().reshape(ref[name].shape)
        assert_grad_close(got, ref[name], f"rowops fold_ln {name}" if name in ("Wf", "bf") else f"rowops unfold_ln {name}")


# --- g. as_group_reduce ---------------------------------------------------------------------------------------------------------
_GR_LENS = [4, 1020, 4 * (1024 * 256) + 4096]   # the last: past the grid cap of 1024 workgroups of 256 float4, into the stride loop


def _group_reduce_ref32(part, src, C):
    """fp32, groups added in index order from 0.0f: what the kernel states"""
    out = np.zeros((C, part.shape[1]), np.float32)
    for g, c in enumerate(src):
        if 0 <= c < C:
            out[c] = out[c] + part[g]
    return out


@pytest.mark.parametrize("length", _GR_LENS)
@pytest.mark.parametrize("G,C", [(1, 1), (5, 1), (12, 1), (1, 3), (5, 3), (12, 3)])
def test_group_reduce(dev, G, C, length):
    """Three group -> channel tables: every group onto one channel (the other channels receive none and must be written as
    zeros), no group onto any channel, and a mixed table.  Bit-equal to the fp32 sum in group order; against float64 the
    error of such a sum is at most (G - 1) roundings of partial sums no larger than sum|part|: (G - 1) 2^-24 sum_g |part_g|."""
    _lib, L = _L()
    rng = np.random.RandomState(G * 10 + C + length % 97)
    part = rng.randn(G, length).astype(np.float32)
    tpart = _dev(part, dev)
    for src in (np.full(G, C - 1), np.full(G, C + 2), rng.randint(0, C, G)):
        src = src.astype(np.int32)
        dst, tsrc = _nan(dev, C + 1, length), _dev(src, dev)
        _lib.check(L.as_group_reduce(_lib.ptr(tpart), _lib.ptr(tsrc), G, C, length, _lib.ptr(dst), _lib.stream_ptr()),
                   "as_group_reduce")
        torch.cuda.synchronize()
        what = f"as_group_reduce G={G} C={C} len={length} src={src.tolist()}"
        _guarded(dst, C, what)
        got = dst[:C].cpu().numpy()
        _same_bits(got, _group_reduce_ref32(part, src, C), what)
        ref = np.stack([part.astype(np.float64)[src == c].sum(0) for c in range(C)])
        bound = max(G - 1, 0) * 2.0 ** -24 * np.stack([np.abs(part.astype(np.float64))[src == c].sum(0) for c in range(C)])
        assert (np.abs(got - ref) <= bound).all(), what
        for c in range(C):
            if not (src == c).any():
                assert (got[c] == 0).all(), f"{what}: channel {c} receives no group and is not zero"


def test_group_reduce_refuses_odd_lengths_and_misaligned_buffers(dev):
    _lib, L = _L()
    part, src, dst = torch.zeros(2 * 64 + 4, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), _nan(dev, 64 + 4)
    st = _lib.stream_ptr()
    _refused(L.as_group_reduce(_lib.ptr(part), _lib.ptr(src), 2, 1, 62, _lib.ptr(dst), st), -1, "as_group_reduce: len % 4 != 0")
    _refused(L.as_group_reduce(_lib.ptr(part[1:]), _lib.ptr(src), 2, 1, 64, _lib.ptr(dst), st), -1, "as_group_reduce: part + 1 float")
    _refused(L.as_group_reduce(_lib.ptr(part), _lib.ptr(src), 2, 1, 64, _lib.ptr(dst[1:]), st), -1, "as_group_reduce: dst + 1 float")
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()


# --- h. element-wise and gather kernels: exact in fp32, bit equality ----------------------------------------------------------
_EW_NS = [1, 1000, GRID_CAP, GRID_CAP + 4321]   # below, at and above what one pass of the capped grid covers


@pytest.mark.parametrize("n", _EW_NS)
def test_add(dev, n):
    _lib, L = _L()
    rng = np.random.RandomState(n % 1000)
    a, b = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    ta, tb, st = _dev(a, dev), _dev(b, dev), _lib.stream_ptr()
    dst = _nan(dev, n + 64)
    _lib.check(L.as_add(_lib.ptr(ta), _lib.ptr(tb), _lib.ptr(dst), n, st), "as_add")
    _guarded(dst, n, "as_add")
    _same_bits(dst[:n], a + b, f"as_add n={n}")
    dst = _nan(dev, n + 64)
    _lib.check(L.as_add(_lib.ptr(ta), None, _lib.ptr(dst), n, st), "as_add")   # b == NULL: a copy
    _guarded(dst, n, "as_add, b = NULL")
    _same_bits(dst[:n], a, f"as_add b=NULL n={n}")
    acc = _nan(dev, n + 64)
    acc[:n] = ta
    _lib.check(L.as_add(_lib.ptr(acc), _lib.ptr(tb), _lib.ptr(acc), n, st), "as_add")   # dst == a
    _guarded(acc, n, "as_add, dst == a")
    _same_bits(acc[:n], a + b, f"as_add in place n={n}")


def test_call_passes_tensors_null_and_the_stream(dev):
    """_lib.call, the way package code enters the library: tensors as their addresses, None as NULL, and the stream appended --
    the current one, the one a torch.cuda.stream block makes current, or the one handed in -- at n = 5, an odd tail.  Then
    _lib.gemm on a 4 x 4 x 4 product against float64."""
    _lib, _ = _L()
    n = 5
    rng = np.random.RandomState(5)
    a, b = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    ta, tb = _dev(a, dev), _dev(b, dev)
    dsts = [_nan(dev, n + 64) for _ in range(4)]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))   # the operands and the NaN fills were enqueued on the current stream
    _lib.call("as_add", ta, tb, dsts[0], n)
    with torch.cuda.stream(side):
        _lib.call("as_add", ta, tb, dsts[1], n)
    _lib.call("as_add", ta, tb, dsts[2], n, stream=side)
    _lib.call("as_add", ta, None, dsts[3], n, stream=side.cuda_stream)   # b == NULL: a copy; a raw stream handle
    side.synchronize()
    for dst, what in zip(dsts[:3], ("current stream", "torch.cuda.stream(side)", "stream=side")):
        _guarded(dst, n, f"call as_add, {what}")
        _same_bits(dst[:n], a + b, f"call as_add, {what}")
    _guarded(dsts[3], n, "call as_add, b = None")
    _same_bits(dsts[3][:n], a, "call as_add, b = None")
    # C = A B^T in exact fp32 products, fp32 accumulation: |error| <= gamma_K sum_k |a b| with gamma_K ~ K 2^-24; twice that allowed
    A, Bm = rng.randn(4, 4).astype(np.float32), rng.randn(4, 4).astype(np.float32)
    tA, tB, out = _dev(A, dev), _dev(Bm, dev), _nan(dev, 16 + 64)
    _lib.gemm(A=tA, B=tB, C=out, M=4, N=4, K=4, a_i=4, a_k=1, b_j=4, b_k=1, ldc=4)
    _guarded(out, 16, "gemm 4 x 4 x 4")
    ref = A.astype(np.float64) @ Bm.astype(np.float64).T
    bound = 2 * 4 * 2.0 ** -24 * float((np.abs(A).astype(np.float64) @ np.abs(Bm).astype(np.float64).T).max())
    _close(out[:16].cpu().numpy().reshape(4, 4), ref, 0.0, bound, "call gemm", "gemm 4 x 4 x 4")


@pytest.mark.parametrize("row_len,rows", [(1, 3), (1, 600001), (50, 5), (50, 11003), (64, 1), (64, 9001), (2816, 3), (2816, 201)])
def test_row_scale(dev, row_len, rows):
    _lib, L = _L()
    rng = np.random.RandomState(row_len + rows % 100)
    a, rs = rng.randn(rows, row_len).astype(np.float32), rng.randn(rows).astype(np.float32)
    dst, ta, trs = _nan(dev, rows + 1, row_len), _dev(a, dev), _dev(rs, dev)
    _lib.check(L.as_row_scale(_lib.ptr(ta), _lib.ptr(trs), _lib.ptr(dst), rows, row_len, _lib.stream_ptr()), "as_row_scale")
    _guarded(dst, rows, "as_row_scale")
    _same_bits(dst[:rows], a * rs[:, None], f"as_row_scale rows={rows} row_len={row_len}")


@pytest.mark.parametrize("n", _EW_NS)
def test_relu_bwd(dev, n):
    """dst = act > 0 ? g : 0 -- +0.0, -0.0 and negatives (a negative denormal among them) drop, a positive denormal keeps"""
    _lib, L = _L()
    rng = np.random.RandomState(n % 1000 + 1)
    g, act = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    act[0::5], act[1::5], act[2::5], act[3::5] = 0.0, -0.0, 1e-40, -1e-40
    dst, tg, tact = _nan(dev, n + 64), _dev(g, dev), _dev(act, dev)
    _lib.check(L.as_relu_bwd(_lib.ptr(tg), _lib.ptr(tact), _lib.ptr(dst), n, _lib.stream_ptr()), "as_relu_bwd")
    _guarded(dst, n, "as_relu_bwd")
    _same_bits(dst[:n], np.where(act > 0, g, np.float32(0)), f"as_relu_bwd n={n}")


@pytest.mark.parametrize("D", [20, 64, 260])
@pytest.mark.parametrize("B,T", [(1, 5), (3, 7), (40, 26)])   # 5, 21 and 1040 rows
def test_embed_posenc(dev, B, T, D):
    """out[m] = table[tokens[b][t]] + pe[t] with m = b T + t and a token row pitch larger than T; table == NULL: out[m] += pe[m % T]"""
    _lib, L = _L()
    rng = np.random.RandomState(B * T + D)
    V, tok_stride, rows = 17, T + 3, B * T
    table, pe = rng.randn(V, D).astype(np.float32), rng.randn(T, D).astype(np.float32)
    tokens = rng.randint(0, V, (B, tok_stride)).astype(np.int64)
    out, ttok, ttab, tpe = _nan(dev, rows + 1, D), _dev(tokens, dev), _dev(table, dev), _dev(pe, dev)
    _lib.check(L.as_embed_posenc(_lib.ptr(ttok), tok_stride, _lib.ptr(ttab), _lib.ptr(tpe), _lib.ptr(out), rows, T, D, _lib.stream_ptr()),
               "as_embed_posenc")
    _guarded(out, rows, "as_embed_posenc")
    want = table[tokens[:, :T].reshape(-1)] + np.tile(pe, (B, 1))
    _same_bits(out[:rows], want, f"as_embed_posenc B={B} T={T} D={D}")
    x = rng.randn(rows, D).astype(np.float32)
    out = _nan(dev, rows + 1, D)
    out[:rows] = _dev(x, dev)
    _lib.check(L.as_embed_posenc(None, 0, None, _lib.ptr(tpe), _lib.ptr(out), rows, T, D, _lib.stream_ptr()), "as_embed_posenc")
    _guarded(out, rows, "as_embed_posenc, table = NULL")
    _same_bits(out[:rows], x + np.tile(pe, (B, 1)), f"as_embed_posenc table=NULL B={B} T={T} D={D}")


# the copy kernel's grid is capped at 4096 workgroups of 256 float4: from 7 x that many float4 on, a lane runs the 8-way unrolled
# loop; 10 x the cap + 1001 float4 gives every lane one unrolled round and then two or three single steps
_COPY_CAP4 = 4096 * 256


@pytest.mark.parametrize("n", [4, 1024, 4 * (10 * _COPY_CAP4 + 1001)])
def test_copy_f32(dev, n):
    _lib, L = _L()
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    src = torch.randn(n, device=dev, generator=g)
    dst = _nan(dev, n + 64)
    _lib.check(L.as_copy_f32(_lib.ptr(src), _lib.ptr(dst), n, _lib.stream_ptr()), "as_copy_f32")
    torch.cuda.synchronize()
    assert torch.isnan(dst[n:]).all()
    assert torch.equal(dst[:n].view(torch.int32), src.view(torch.int32))   # bits


def test_copy_f32_refuses_lengths_that_are_no_multiple_of_4(dev):
    _lib, L = _L()
    src, dst = torch.zeros(8, device=dev), _nan(dev, 8)
    _refused(L.as_copy_f32(_lib.ptr(src), _lib.ptr(dst), 6, _lib.stream_ptr()), -1, "as_copy_f32: n % 4 != 0")
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()


def _dropout_keep(seed, n, p):
    """The generator as rowops.hip states it, in uint64: z = seed + (i + 1) 0x9E3779B97F4A7C15, the splitmix64 finaliser, the
    top 24 bits as u in [0, 1); element i is kept iff u >= p"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_fwd_matches_the_stated_generator(dev, p):
    """as_dropout_fwd over two passes of the capped grid and 77 elements more: kept / dropped pattern and the scale
    1 / (1 - p) bit for bit; p = 0 is the identity"""
    _lib, L = _L()
    n, seed = GRID_CAP * 2 + 77, 0x1234_5678_9ABC_DEF1
    x = (np.random.RandomState(9).randn(n).astype(np.float32))
    y, tx = _nan(dev, n + 64), _dev(x, dev)
    _lib.check(L.as_dropout_fwd(_lib.ptr(tx), _lib.ptr(y), n, p, seed, _lib.stream_ptr()), "as_dropout_fwd")
    _guarded(y, n, "as_dropout_fwd")
    keep = _dropout_keep(seed, n, p)
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    _same_bits(y[:n], x * np.where(keep, inv_keep, np.float32(0)), f"as_dropout_fwd p={p}")
    if p == 0.0:
        _same_bits(y[:n], x, "as_dropout_fwd p=0 is the identity")
    else:
        assert abs(keep.mean() - (1 - p)) < 3e-3   # 4 sigma at n = 1e6 is 2e-3


def test_dropout_fwd_refuses_p_of_one(dev):
    _lib, L = _L()
    x, y = torch.ones(8, device=dev), _nan(dev, 8)
    _refused(L.as_dropout_fwd(_lib.ptr(x), _lib.ptr(y), 8, 1.0, 3, _lib.stream_ptr()), -1, "as_dropout_fwd: p = 1")
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
