"""The float64 restatements of tests/scorer_kernels_fp64.py (no GPU): each equals F.conv2d / F.layer_norm + F.gelu / autograd in
float64 on the reference layout (B, C, D, T) to 1e-12, and the checker `compare` fails for every defect a convolution kernel of
this shape can have (planted into torch's own float32 result) while passing for that result untouched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scorer_kernels_fp64 as K


def _close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1.0), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("B,T,D,Ci,Co", [(1, 1, 1, 32, 32), (2, 5, 7, 32, 32), (2, 3, 1, 3, 32), (1, 4, 2, 6, 5)])
def test_conv3x3_cl_is_conv2d_on_the_reference_layout(B, T, D, Ci, Co):
    g = torch.Generator().manual_seed(B + T + D)
    x = torch.randn(B, T, D, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64)
    bias, res = torch.randn(Co, generator=g, dtype=torch.float64), torch.randn(B, T, D, Co, generator=g, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 2, 1), w, bias, padding=1).permute(0, 3, 2, 1)
    taps = w.permute(2, 3, 0, 1)
    _close(K.conv3x3_cl(x, taps, bias), want)
    _close(K.conv3x3_cl(x, taps, bias, res), want + res)
    _close(K.conv3x3_cl(x.float(), taps.float(), bias.float()), F.conv2d(x.float().double().permute(0, 3, 2, 1), w.float().double(),
                                                                         bias.float().double(), padding=1).permute(0, 3, 2, 1))


@pytest.mark.parametrize("B,T,D", [(1, 1, 1), (2, 5, 7), (1, 3, 2)])
def test_flipped_taps_give_the_data_gradient(B, T, D):
    """w'[kd][kt][ci][co] = w[2 - kd][2 - kt][co][ci] (DeepSpeech2._prepare_bwd): conv3x3_cl(dy, w', 0) is autograd's dx."""
    g = torch.Generator().manual_seed(7 * B + T + D)
    w = torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(B, T, D, 32, generator=g, dtype=torch.float64)
    x = torch.zeros(B, 32, D, T, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, padding=1).backward(dy.permute(0, 3, 2, 1))
    flipped = w.flip(2, 3).transpose(0, 1).permute(2, 3, 0, 1)
    _close(K.conv3x3_cl(dy, flipped, torch.zeros(32)), x.grad.permute(0, 3, 2, 1))


@pytest.mark.parametrize("layout", ["plain", "rows", "padded"])
@pytest.mark.parametrize("Cin,voiced", [(1, True), (2, False), (6, True)])
def test_stem_reads_through_the_strides(layout, Cin, voiced):
    B, T, D = 2, 5, 3
    g = torch.Generator().manual_seed(Cin)
    x = torch.randn(B, Cin, D, T, generator=g, dtype=torch.float64)
    planes, strides = K.stem_planes(x, layout)
    w = torch.randn(32, Cin, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(32, generator=g, dtype=torch.float64)
    v = torch.randn(B, T, generator=g, dtype=torch.float64) if voiced else None
    want = F.conv2d(x, w, bias, padding=1)
    if voiced:
        want = want + v[:, None, None, :]
    _close(K.stem(planes, strides, w.permute(2, 3, 0, 1), bias, v, (B, T, D)), want.permute(0, 3, 2, 1))


@pytest.mark.parametrize("rows,D,C", [(1, 1, 32), (3, 7, 32), (2, 81, 4)])
def test_ln_feat_gelu_and_its_gradient_are_torchs(rows, D, C):
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(rows, D, C, generator=g, dtype=torch.float64) * 2 + 0.3).requires_grad_(True)
    gamma, beta = torch.rand(D, generator=g, dtype=torch.float64) + 0.5, torch.randn(D, generator=g, dtype=torch.float64) * 0.2
    dy = torch.randn(rows, D, C, generator=g, dtype=torch.float64)
    want = F.gelu(F.layer_norm(x.transpose(1, 2), (D,), gamma, beta, 1e-5)).transpose(1, 2)
    got = K.ln_feat_gelu(x, gamma, beta)
    _close(got, want)
    gw, = torch.autograd.grad(want, x, dy)
    gg, = torch.autograd.grad(got, x, dy)
    _close(gg, gw)


def test_gelu_and_gelu_bwd_are_torchs():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(5, 48, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    dy, scale = torch.randn(5, 48, generator=g, dtype=torch.float64), torch.randn(48, generator=g, dtype=torch.float64)
    _close(K.gelu(x), F.gelu(x))
    gx, = torch.autograd.grad(F.gelu(x), x, dy)
    _close(K.gelu_bwd(dy, x), gx)
    _close(K.gelu_bwd(dy, x, scale, 48), gx * scale[None, :])
    _close(K.gelu_bwd(dy, x, scale[:1], 1), gx * scale[0])
    gs, = torch.autograd.grad(K.gelu(x), x, dy)
    _close(gs, gx)


# ------------------------------------------------------------------------------------------- what `compare` can and cannot miss
def _neighbour_rows(x, taps, kd):
    """Contribution of the taps (kd, all kt) read at flattened position q + (kt - 1) * D + (kd - 1) of the utterance, whatever
    feature that position belongs to: what a kernel adds when it does not treat the feature-axis edge as padding."""
    B, T, D, _ = x.shape
    flat = x.reshape(B, T * D, 32)
    out = torch.zeros(B, T * D, 32)
    q = torch.arange(T * D)
    for kt in range(3):
        src = q + (kt - 1) * D + (kd - 1)
        ok = (src >= 0) & (src < T * D)
        out[:, ok] += flat[:, src[ok]] @ taps[kd, kt].t()
    return out.reshape(B, T, D, 32)


def _planted(case, defect, fill):
    """torch's float32 result (with the residual) carrying one defect of a tiled implicit-GEMM convolution."""
    x, taps, res = case["x"], case["taps"], case["res"]
    B, T, D, _ = x.shape
    y = case["ref32_res"].clone()
    tail = T * D - T * D % 128   # first row of the last, partial 128-row tile of every utterance
    if defect == "wrap_low":      # d = 0: the kd = -1 neighbour is the previous frame's last feature, not zero
        y[:, :, 0] += _neighbour_rows(x, taps, 0)[:, :, 0]
    elif defect == "wrap_high":   # d = D - 1: the kd = +1 neighbour is the next frame's first feature
        y[:, :, D - 1] += _neighbour_rows(x, taps, 2)[:, :, D - 1]
    elif defect == "last_frame":  # the kt = +1 taps never see the last frame
        y[:, T - 2] -= K.conv3x3_cl(x[:, T - 1:], torch.stack([torch.zeros_like(taps[:, 0]), taps[:, 2], torch.zeros_like(taps[:, 0])], 1),
                                    torch.zeros(32)).float()[:, 0]
    elif defect == "no_res_tail":  # the residual is not added on the rows of the partial tile
        y.view(B, T * D, 32)[:, tail:] -= res.view(B, T * D, 32)[:, tail:]
    elif defect == "unwritten_tail":  # the partial tile is not stored
        y.view(B, T * D, 32)[:, tail:] = fill
    return y


DEFECT_SHAPES = [(2, 20, 15), (2, 19, 16), (2, 4, 95), (2, 3, 176), (2, 9, 16), (2, 150, 2), (2, 300, 1)]


@pytest.mark.parametrize("defect", ["wrap_low", "wrap_high", "last_frame", "no_res_tail", "unwritten_tail"])
@pytest.mark.parametrize("B,T,D", DEFECT_SHAPES)
def test_compare_fails_for_every_planted_defect(defect, B, T, D):
    """Of the defects, "last_frame" is stated for the frame that HAS a successor: on the last output frame the kt = +1 taps read
    padding in a correct kernel too, so dropping them there changes nothing; what a kernel can get wrong is whether the last
    frame's rows reach the taps of the frame before it."""
    assert (B, T, D) in K.C32_SHAPES and T * D % 128
    case = K.c32_case(B, T, D)
    for fill in ((float("nan"), 0.0) if defect == "unwritten_tail" else (None,)):
        bad = _planted(case, defect, fill)
        assert not torch.equal(bad, case["ref32_res"])
        with pytest.raises(AssertionError, match="max err"):
            K.compare(bad, case["ref_res"], case["ref32_res"], f"planted {defect}")
    K.WORST.pop(f"planted {defect}", None)


@pytest.mark.parametrize("B,T,D", K.C32_SHAPES)
def test_compare_passes_for_torchs_float32_at_every_shape(B, T, D):
    """The bound is satisfiable at every shape the GPU test runs: torch's float32 result passes, and is not exact."""
    case = K.c32_case(B, T, D)
    for sfx in ("", "_res"):
        ratio = K.compare(case["ref32" + sfx], case["ref" + sfx], case["ref32" + sfx], "host self-check")
        assert ratio == 1.0 and float((case["ref32" + sfx].double() - case["ref" + sfx]).abs().max()) > 0
    K.WORST.pop("host self-check", None)
