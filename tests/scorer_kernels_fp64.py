"""float64 restatements of the recogniser's forward and input-gradient kernels (csrc/conv.hip) in the kernels' own layouts, and
the checker the kernel tests share.  Plain torch on the host: every function takes tensors of any float dtype and computes in
float64; all of them are differentiable, so autograd over a restatement is the float64 truth of the matching backward kernel.

    conv3x3_cl    as_conv3x3_c32 (and the stem's arithmetic): channels-last maps x[B][T][D][Ci], taps[kd][kt][co][ci]
    stem          as_conv3x3_stem: planar input read through explicit element strides, optional per-(b, t) voicing bias
    ln_feat_gelu  as_ln_feat_gelu: LayerNorm over the feature axis of x[rows][D][C], then exact GELU
    gelu, gelu_bwd   as_gelu, as_gelu_bwd (optional per-column scale: i -> scale[i % row_len])
    compare       max|got - ref| <= 2 * max|ref32 - ref| + 1e-6 * max|ref|: the bound form of the CTC tests (_check_ctc)
"""
import math

import numpy as np
import torch

from conftest import WORST

F64 = torch.float64


def conv3x3_cl(x, taps, bias, res=None):
    """y[b][t][d][co] = bias[co] + sum_{kd, kt, ci} taps[kd][kt][co][ci] * x[b][t + kt - 1][d + kd - 1][ci] (zero outside the map)
    [+ res[b][t][d][co]]."""
    x, taps = x.to(F64), taps.to(F64)
    B, T, D, Ci = x.shape
    assert taps.shape[:2] == (3, 3) and taps.shape[3] == Ci, (taps.shape, x.shape)
    pad = x.new_zeros(B, T + 2, D + 2, Ci)
    pad[:, 1:T + 1, 1:D + 1] = x
    y = bias.to(F64).expand(B, T, D, taps.shape[2]).clone()
    for kd in range(3):
        for kt in range(3):
            y = y + pad[:, kt:kt + T, kd:kd + D] @ taps[kd, kt].t()
    return y if res is None else y + res.to(F64)


def stem(planes, strides, taps, bias, voicing, shape):
    """planes: a flat buffer, element (b, ci, d, t) at planes[b * sb + ci * sc + d * sd + t * st] with strides = (sb, sc, sd, st);
    shape = (B, T, D); taps[kd][kt][32][Cin]; voicing (B, T) or None is added to every channel of frame (b, t)."""
    B, T, D = shape
    Cin = taps.shape[3]
    x = torch.as_strided(planes.to(F64).reshape(-1), (B, Cin, D, T), tuple(strides))
    y = conv3x3_cl(x.permute(0, 3, 2, 1), taps, bias)
    return y if voicing is None else y + voicing.to(F64)[:, :, None, None]


def stem_planes(x, layout):
    """x (B, C, D, T) -> (flat buffer, element strides) in the plain (B, C, D, T) layout, the adapter's (B, C, T, D) rows, or those
    rows at a padded plane pitch (the padding holds NaN: nothing may read it)."""
    B, C, D, T = x.shape
    if layout == "plain":
        return x.contiguous().reshape(-1), (C * D * T, D * T, T, 1)
    if layout == "rows":
        return x.transpose(2, 3).contiguous().reshape(-1), (C * T * D, T * D, 1, D)
    pitch = T * D + 5
    buf = torch.full((B, C, pitch), float("nan"), dtype=x.dtype)
    buf[:, :, :T * D] = x.transpose(2, 3).reshape(B, C, T * D)
    return buf.reshape(-1), (C * pitch, pitch, 1, D)


def gelu(x):
    x = x.to(F64)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    x = x.to(F64)
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_bwd(dy, x, scale=None, row_len=0):
    """dx[i] = dy[i] * gelu'(x[i]) [* scale[i % row_len]] over the flattened tensors."""
    g = dy.to(F64).reshape(-1) * gelu_grad(x.reshape(-1))
    if scale is not None:
        g = g * scale.to(F64)[torch.arange(g.numel()) % row_len]
    return g.reshape(dy.shape)


def ln_feat_gelu(x, gamma, beta, eps=1e-5):
    """y[r][d][c] = gelu((x[r][d][c] - mean_d) / sqrt(var_d + eps) * gamma[d] + beta[d]), statistics over d for every (r, c)
    (biased variance)."""
    x = x.to(F64)
    mean = x.mean(dim=1, keepdim=True)
    e = x - mean
    var = (e * e).mean(dim=1, keepdim=True)
    return gelu(e / torch.sqrt(var + eps) * gamma.to(F64)[None, :, None] + beta.to(F64)[None, :, None])


# ---------------------------------------------------------------------------------------------- the shapes of as_conv3x3_c32
# Feature widths at which its launcher changes the LDS image: the halo row count ceil((130 + 2 D) / 160) * 160 steps at
# D = 15 -> 16 and 95 -> 96, the halo stops fitting in 64 KB at 175 -> 176 (conv3x3_mfma_kernel takes over); 1 and 2 are the
# widths at which both feature-axis edges meet in one or two positions.
C32_WIDTHS = (1, 2, 15, 16, 95, 96, 175, 176, 200)


def _ragged_frames(D):
    """The smallest T >= 3 with T * D >= 300 (more than two 128-row tiles per utterance) and T * D no multiple of 128."""
    T = max(3, -(-300 // D))
    while T * D % 128 == 0:
        T += 1
    return T


# (B, T, D): every width with a ragged last tile and with a single frame; one and two whole tiles per utterance, a whole tile plus
# a partial one, a single position; more tiles (3 * 172) than the persistent grid of 512 workgroups
C32_SHAPES = tuple((2, _ragged_frames(D), D) for D in C32_WIDTHS) + tuple((2, 1, D) for D in C32_WIDTHS) + (
    (2, 8, 16), (2, 64, 2), (2, 9, 16), (1, 1, 1), (3, 1375, 16))

_c32_cases = {}


def c32_case(B, T, D):
    """Inputs of one as_conv3x3_c32 call (float32, seeded by the shape) with the float64 truth and torch's own float32 CPU result
    (F.conv2d on the reference layout (B, C, D, T)), without and with the residual input.  Computed once per shape."""
    key = (B, T, D)
    if key not in _c32_cases:
        import torch.nn.functional as F
        g = torch.Generator().manual_seed(1000 * D + 10 * T + B)
        x, res = torch.randn(B, T, D, 32, generator=g), torch.randn(B, T, D, 32, generator=g)
        w = torch.randn(32, 32, 3, 3, generator=g) / math.sqrt(288.0)
        bias = torch.randn(32, generator=g)
        taps = w.permute(2, 3, 0, 1).contiguous()   # [kd][kt][co][ci]
        ref = conv3x3_cl(x, taps, bias)
        ref32 = F.conv2d(x.permute(0, 3, 2, 1), w, bias, padding=1).permute(0, 3, 2, 1).contiguous()
        _c32_cases[key] = dict(x=x, res=res, w=w, taps=taps, bias=bias, ref=ref, ref32=ref32, ref_res=ref + res.double(),
                               ref32_res=ref32 + res)
    return _c32_cases[key]


def compare(got, ref, ref32, label):
    """got within twice torch's own float32 error of the float64 truth, plus 1e-6 of the tensor's maximum.  ref32 is torch's
    float32 CPU result on the same inputs.  The ratio err / err32 goes to WORST[label] (conftest.py writes it out with the other worst errors at
    the end of a GPU session).
    A NaN anywhere in got fails."""
    a, r, r32 = (np.asarray(torch.as_tensor(v).detach().cpu(), np.float64) for v in (got, ref, ref32))
    assert a.shape == r.shape == r32.shape, (label, a.shape, r.shape, r32.shape)
    scale = max(float(np.abs(r).max()), 1e-30)
    err, err32 = float(np.abs(a - r).max()), float(np.abs(r32 - r).max())
    ratio = err / max(err32, 1e-30)
    WORST[label] = ratio if math.isnan(ratio) else max(WORST.get(label, 0.0), ratio)
    assert err <= 2 * err32 + 1e-6 * scale, f"{label}: max err {err:.3e} > 2 x torch fp32's {err32:.3e} + 1e-6 * {scale:.3e}"
    return ratio
