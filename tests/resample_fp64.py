"""The polyphase windowed-sinc resampler restated for the tests (no engine code): the dense filter table with plain loops and the
math module from the formulas (sinc_interp_hann and sinc_interp_kaiser, I0 by its power series), the float64 oracle
y[j n + i] = sum_k h[i][k] xz[j o + k - width] with zero padding, cut to (n L + o - 1) // o samples, and the *stock fp32 path*:
torch.nn.functional.conv1d with stride o in float32 on the CPU over the float32-rounded dense table, which is what
torchaudio's formulation runs."""
import functools
import math

import torch

KAISER_BETA = 14.769656459379492
# (orig, new): 3 -> 2, 2 -> 3, 7 -> 5, one phase, 160 phases, 320 phases, 441 phases (upsampling)
RATIOS = [(3, 2), (2, 3), (7, 5), (48000, 16000), (44100, 16000), (22050, 16000), (16000, 44100)]
METHODS = ["sinc_interp_hann", "sinc_interp_kaiser"]


def bessel_i0(x):
    """I0(x) = sum_k ((x / 2)^k / k!)^2; converged to float64 for the |x| <= 40 the windows use"""
    total, term, k = 1.0, 1.0, 0
    while term > 1e-18 * total:
        k += 1
        term *= (x / 2.0 / k) ** 2
        total += term
    return total


def ratio(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


@functools.lru_cache(maxsize=None)
def dense_table(orig, new, method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, beta=None):
    """(h (n, 2 width + o) float64, width)"""
    o, n = ratio(orig, new)
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    K = 2 * width + o
    beta = KAISER_BETA if beta is None else beta
    h = torch.zeros(n, K, dtype=torch.float64)

    def tap(t):
        if method == "sinc_interp_hann":
            window = math.cos(t * math.pi / lowpass_filter_width / 2) ** 2
        else:
            window = bessel_i0(beta * math.sqrt(max(0.0, 1 - (t / lowpass_filter_width) ** 2))) / bessel_i0(beta)
        sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
        return sinc * window * base / o

    rim = tap(float(lowpass_filter_width))   # the clamped argument: most taps of a dense row (even in t)
    for i in range(n):
        row = []
        for k in range(K):
            t = (-i / n + (k - width) / o) * base
            t = max(-lowpass_filter_width, min(lowpass_filter_width, t))
            row.append(rim if abs(t) == lowpass_filter_width else tap(t))
        h[i] = torch.tensor(row, dtype=torch.float64)
    return h, width


def target_length(L, orig, new):
    o, n = ratio(orig, new)
    return (n * L + o - 1) // o


def resample(x, orig, new, dtype=torch.float64, **kw):
    """the 1-D signal x resampled on the CPU: the dense strided convolution in `dtype` over the table rounded to `dtype`"""
    o, n = ratio(orig, new)
    h, width = dense_table(orig, new, **kw)
    x = x.detach().cpu().to(dtype)
    L = len(x)
    padded = torch.nn.functional.pad(x, (width, width + o))
    y = torch.nn.functional.conv1d(padded[None, None], h.to(dtype)[:, None], stride=o)   # (1, n, J)
    return y[0].t().reshape(-1)[:target_length(L, orig, new)]


def band_of(h, threshold=1e-20):
    """(first, last) tap above the threshold, per phase"""
    live = h.abs() > threshold
    K = h.shape[1]
    taps = torch.arange(K)
    return torch.where(live, taps, K).min(dim=1).values, torch.where(live, taps, -1).max(dim=1).values


def test_signal(n, seed, rate_fraction=0.11):
    """0.5 sin(2 pi f t) + 0.3 sin(2 pi 2.7 f t + 1) + 0.01 N(0, 1) with f = rate_fraction / 2.7 cycles per sample, float32, rounded
    to the int16 grid (k / 32768), so that the same values exist as int16"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    f = rate_fraction / 2.7
    x = 0.5 * torch.sin(2 * math.pi * f * t) + 0.3 * torch.sin(2 * math.pi * 2.7 * f * t + 1.0)
    x = x + 0.01 * torch.randn(n, generator=g, dtype=torch.float64)
    return (torch.round(x * 32768.0).clamp(-32768, 32767) / 32768.0).float()
