"""The recogniser's kernels one by one (csrc/conv.hip, csrc/scorer_wgrad.hip) against the float64 restatements of
tests/scorer_kernels_fp64.py, at every shape where a launcher changes kernel, tile count or LDS image.  The C ABI is called as
deepspeech2.py calls it (_lib.call, None for a null pointer); every output starts as NaN inside a larger buffer whose guard
words must survive the launch."""
import math

import pytest
import torch
import torch.nn.functional as F

import scorer_kernels_fp64 as K
from conftest import WORST, assert_grad_close

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 1024, 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def _call(name, *args):
    from artspeech_amd import _lib
    _lib.call(name, *args)


def _guarded(n, dev):
    """(buffer, the n floats of it an output goes to): NaN inside, GUARD sentinel floats either side."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    buf[:GUARD] = SENTINEL
    buf[GUARD + n:] = SENTINEL
    return buf, buf[GUARD:GUARD + n]


def _written_exactly(buf, n, what):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), f"{what}: wrote outside its output"
    assert not bool(torch.isnan(buf[GUARD:GUARD + n]).any()), f"{what}: left output elements unwritten"


def _within(got, ref, frac, label):
    """max|got - ref| <= frac * max|ref| (the bound form of test_ln_feat_gelu_bwd_matches_fp64); the observed fraction goes to WORST."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    WORST[label] = max(WORST.get(label, 0.0), err / max(scale, 1e-30))
    assert err <= frac * scale, f"{label}: max err {err:.3e} > {frac:g} * {scale:.3e}"


# ------------------------------------------------------------------------------------------------------- as_conv3x3_c32
def _c32(x, taps, bias, res, B, T, D, dev, what):
    """Two launches into fresh guarded buffers: bit-identical, everything written, nothing else touched."""
    xd, td, bd = x.to(dev), taps.to(dev), bias.to(dev)
    rd = res.to(dev) if res is not None else None
    n = B * T * D * 32
    runs = []
    for _ in range(2):
        buf, y = _guarded(n, dev)
        _call("as_conv3x3_c32", xd, td, bd, rd, y, B, T, D)
        _written_exactly(buf, n, what)
        runs.append(y.cpu())
    assert torch.equal(runs[0], runs[1]), f"{what}: two launches differ"
    return runs[0].view(B, T, D, 32)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("B,T,D", K.C32_SHAPES)
def test_conv3x3_c32_matches_fp64(B, T, D, with_res, dev):
    case = K.c32_case(B, T, D)
    what = f"conv3x3_c32 B={B} T={T} D={D}" + (" +res" if with_res else "")
    got = _c32(case["x"], case["taps"], case["bias"], case["res"] if with_res else None, B, T, D, dev, what)
    sfx = "_res" if with_res else ""
    K.compare(got, case["ref" + sfx], case["ref32" + sfx], what + " / torch fp32")


@pytest.mark.parametrize("D", [2, 16, 176])
def test_conv3x3_c32_over_flipped_taps_is_the_data_gradient(D, dev):
    """DeepSpeech2._prepare_bwd's operands: w'[kd][kt][ci][co] = w[2 - kd][2 - kt][co][ci] and a zero bias."""
    B, T = 2, K._ragged_frames(D)
    case = K.c32_case(B, T, D)
    w, dy = case["w"], case["res"]
    grads = {}
    for dt in (torch.float64, torch.float32):
        x = torch.zeros(B, 32, D, T, dtype=dt, requires_grad=True)
        F.conv2d(x, w.to(dt), padding=1).backward(dy.to(dt).permute(0, 3, 2, 1))
        grads[dt] = x.grad.permute(0, 3, 2, 1)
    flipped = w.flip(2, 3).transpose(0, 1).permute(2, 3, 0, 1).contiguous()
    what = f"conv3x3_c32 dx D={D}"
    got = _c32(dy, flipped, torch.zeros(32), None, B, T, D, dev, what)
    K.compare(got, grads[torch.float64], grads[torch.float32], what + " / torch fp32")


# ------------------------------------------------------------------------------------------------------ as_conv3x3_stem
# B * T * D = 255, 256, 257 around the 256-position tile of conv3x3_stem_kernel (and the 8-position blocks of
# conv3x3_small_kernel), and a single frame
STEM_SHAPES = ((3, 5, 17), (2, 8, 16), (1, 257, 1), (2, 1, 5))


@pytest.mark.parametrize("layout", ["plain", "rows", "padded"])
@pytest.mark.parametrize("Cin", [1, 2, 3, 4, 6])   # 4 and 6: conv3x3_small_kernel
def test_conv3x3_stem_matches_fp64(Cin, layout, dev):
    for B, T, D in STEM_SHAPES:
        g = torch.Generator().manual_seed(100 * Cin + B * T * D)
        x = torch.randn(B, Cin, D, T, generator=g)
        w = torch.randn(32, Cin, 3, 3, generator=g) / math.sqrt(9.0 * Cin)
        bias, voicing = torch.randn(32, generator=g), torch.randn(B, T, generator=g)
        taps = w.permute(2, 3, 0, 1).contiguous()
        planes, strides = K.stem_planes(x, layout)
        pd, td, bd, vd = planes.to(dev), taps.to(dev), bias.to(dev), voicing.to(dev)
        n = B * T * D * 32
        for v, v_dev in ((None, None), (voicing, vd)):
            what = f"conv3x3_stem Cin={Cin} {layout} B={B} T={T} D={D}" + (" +voicing" if v is not None else "")
            buf, y = _guarded(n, dev)
            _call("as_conv3x3_stem", pd, *strides, td, bd, v_dev, y, B, T, D, Cin)
            _written_exactly(buf, n, what)
            ref = K.stem(planes, strides, taps, bias, v, (B, T, D))
            ref32 = F.conv2d(x, w, bias, padding=1)
            if v is not None:
                ref32 = ref32 + v[:, None, None, :]
            K.compare(y.cpu().view(B, T, D, 32), ref, ref32.permute(0, 3, 2, 1), f"conv3x3_stem Cin={Cin} {layout} / torch fp32")


# ------------------------------------------------------------------------------- as_ln_feat_gelu, as_ln_feat_gelu_bwd
# D: one feature; 80 / 81 and 128 / 129, the register kernels' widths (forward <80>, <128>, loop; backward <80>, loop); 200.
# rows * 32 columns = 224, 256, 288: short of, exactly and past one 256-thread block
@pytest.mark.parametrize("rows", [7, 8, 9])
@pytest.mark.parametrize("D", [1, 80, 81, 128, 129, 200])
def test_ln_feat_gelu_and_bwd_match_fp64(D, rows, dev):
    g = torch.Generator().manual_seed(10 * D + rows)
    x = torch.randn(rows, D, 32, generator=g) * 2 + 0.3
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.2
    dy, res = torch.randn(rows, D, 32, generator=g), torch.randn(rows, D, 32, generator=g)
    xd, gd, bd, dyd, resd = (t.to(dev) for t in (x, gamma, beta, dy, res))
    n = x.numel()
    x64 = x.double().requires_grad_(True)
    ref = K.ln_feat_gelu(x64, gamma, beta)
    buf, y = _guarded(n, dev)
    _call("as_ln_feat_gelu", xd, gd, bd, y, rows, D, 32)
    _written_exactly(buf, n, f"ln_feat_gelu D={D} rows={rows}")
    _within(y.view(rows, D, 32), ref, 1e-5, f"ln_feat_gelu D={D}")
    dx64, = torch.autograd.grad(ref, x64, dy.double())
    for r, r_dev in ((None, None), (res, resd)):
        what = f"ln_feat_gelu_bwd D={D}" + (" +res" if r is not None else "")
        buf, dx = _guarded(n, dev)
        _call("as_ln_feat_gelu_bwd", xd, gd, bd, dyd, r_dev, dx, rows, D, 32)
        _written_exactly(buf, n, f"{what} rows={rows}")
        _within(dx.view(rows, D, 32), dx64 + (r.double() if r is not None else 0), 1e-5, what)


# ------------------------------------------------------------------------------------------------- as_gelu, as_gelu_bwd
# n = 2048 * 256 + 3 is past the grid cap of as_ew_grid (2048 blocks of 256): the grid-stride loops take a second pass
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
def test_gelu_and_gelu_bwd_match_fp64(n, dev):
    g = torch.Generator().manual_seed(n)
    x, dy = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    scale = torch.randn(48, generator=g)
    xd, dyd, sd = x.to(dev), dy.to(dev), scale.to(dev)
    buf, y = _guarded(n, dev)
    _call("as_gelu", xd, y, n)
    _written_exactly(buf, n, f"gelu n={n}")
    K.compare(y, K.gelu(x), F.gelu(x), "gelu / torch fp32")
    x32 = x.clone().requires_grad_(True)
    g32, = torch.autograd.grad(F.gelu(x32), x32, dy)
    for row_len in (0, 1, 48):   # 0: no scale
        s, s_dev = (scale[:row_len], sd[:row_len].contiguous()) if row_len else (None, None)
        ref = K.gelu_bwd(dy, x, s, row_len)
        ref32 = g32 * s[torch.arange(n) % row_len] if row_len else g32
        buf, dx = _guarded(n, dev)
        _call("as_gelu_bwd", dyd, xd, s_dev, dx, n, row_len)
        _written_exactly(buf, n, f"gelu_bwd n={n} row_len={row_len}")
        K.compare(dx, ref, ref32, f"gelu_bwd row_len={row_len} / torch fp32")
        inplace = dyd.clone()   # dy is dx
        _call("as_gelu_bwd", inplace, xd, s_dev, inplace, n, row_len)
        assert torch.equal(inplace, dx), f"gelu_bwd n={n} row_len={row_len}: in place differs"


# ------------------------------------------------------------------- as_ln_feat_gelu_param_grad, as_layernorm_param_grad
def _slab(dev):
    from artspeech_amd.phoneme_recognition.deepspeech2 import _slab
    return _slab(dev)


def _twice(dev, D, launch):
    """(dgamma, dbeta) of two launches into NaN-filled outputs: bit-identical."""
    runs = []
    for _ in range(2):
        dg, db = torch.full((D,), float("nan"), device=dev), torch.full((D,), float("nan"), device=dev)
        launch(dg, db)
        runs.append((dg.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
    return runs[0]


@pytest.mark.parametrize("rows", [1, 255, 256, 257])   # the split into at most 256 row chunks: 1 row each up to 256, then 2
@pytest.mark.parametrize("D", [128, 129])               # the feature tile LN_DT = 128: one tile, and a second with one feature
def test_ln_feat_gelu_param_grad_matches_fp64(D, rows, dev):
    g = torch.Generator().manual_seed(D + rows)
    x, dy = torch.randn(rows, D, 32, generator=g), torch.randn(rows, D, 32, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    slab = _slab(dev)
    xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    dg, db = _twice(dev, D, lambda dg, db: _call("as_ln_feat_gelu_param_grad", xd, gd, bd, dyd, rows, D, 32, dg, db, slab, slab.numel()))
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    (K.ln_feat_gelu(x, g64, b64) * dy.double()).sum().backward()
    assert_grad_close(dg, g64.grad, f"ln_feat dgamma D={D} rows={rows}", rtol=1e-4, atol_frac=1e-5)
    assert_grad_close(db, b64.grad, f"ln_feat dbeta D={D} rows={rows}", rtol=1e-4, atol_frac=1e-5)


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
@pytest.mark.parametrize("D", [256, 257])               # ln_rows_param_grad_kernel's 256-column tile
def test_layernorm_param_grad_matches_fp64(D, rows, dev):
    g = torch.Generator().manual_seed(D + rows)
    xh, dz = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    slab = _slab(dev)
    dzd, xhd = dz.to(dev), xh.to(dev)
    dg, db = _twice(dev, D, lambda dg, db: _call("as_layernorm_param_grad", dzd, xhd, rows, D, dg, db, slab, slab.numel()))
    assert_grad_close(dg, (dz.double() * xh.double()).sum(0), f"row LN dgamma D={D} rows={rows}")
    assert_grad_close(db, dz.double().sum(0), f"row LN dbeta D={D} rows={rows}")
