"""The mel spectrogram restated for the tests (no engine code): the float64 oracle -- torch.stft on the CPU (centred, reflect
padding, periodic Hann window placed in the middle of the frame, one-sided), the power spectrum, the float64 HTK filterbank and
log(clamp(., clip)) -- and the *stock fp32 path*, the same steps in float32 with a float32 filterbank, which is what the
reference's host code computes.  The filterbank is restated here with plain loops from the formulas, independently of
artspeech_amd.phoneme_recognition.features.mel_filterbank."""
import math

import torch

CLIP = 1e-5
CONFIGS = [(64, 48, 16, 8), (256, 256, 64, 20), (1024, 1024, 256, 80), (2048, 1024, 512, 40)]   # n_fft, win_length, hop, n_mels
SAMPLE_RATE = 16000


def filterbank_fp64(n_freqs, f_min, f_max, n_mels, sample_rate):
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)   # noqa: E731
    nyquist = sample_rate // 2
    freqs = [nyquist * k / (n_freqs - 1) for k in range(n_freqs)]
    lo, hi = mel(f_min), mel(f_max)
    pts = [700.0 * (10.0 ** ((lo + (hi - lo) * i / (n_mels + 1)) / 2595.0) - 1.0) for i in range(n_mels + 2)]
    fb = torch.zeros(n_freqs, n_mels, dtype=torch.float64)
    for k, f in enumerate(freqs):
        for m in range(n_mels):
            fb[k, m] = max(0.0, min((f - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1])))
    return fb


def window_fp64(n_fft, win_length):
    w = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    i = torch.arange(win_length, dtype=torch.float64)
    w[left:left + win_length] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * i / win_length)
    return w


def mel_power(x, n_fft, win_length, hop, n_mels, dtype, sample_rate=SAMPLE_RATE):
    """(n_mels, 1 + n // hop) power mel spectrogram of the 1-D signal x, every step in `dtype` on the CPU"""
    x = x.detach().cpu().to(dtype)
    window = torch.hann_window(win_length, periodic=True, dtype=dtype)
    spec = torch.stft(x, n_fft, hop_length=hop, win_length=win_length, window=window, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    power = spec.abs().pow(2)
    fb = filterbank_fp64(n_fft // 2 + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate).to(dtype)
    return torch.matmul(power.transpose(0, 1), fb).transpose(0, 1)


def log_mel(x, n_fft, win_length, hop, n_mels, dtype, clip=CLIP):
    return torch.log(torch.clamp(mel_power(x, n_fft, win_length, hop, n_mels, dtype), min=clip))


def test_signal(n, seed, sample_rate=SAMPLE_RATE):
    """0.5 sin(2 pi 440 t) + 0.3 sin(2 pi 3000.5 t + 1) + 0.01 N(0, 1), float32"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sample_rate
    x = 0.5 * torch.sin(2 * math.pi * 440.0 * t) + 0.3 * torch.sin(2 * math.pi * 3000.5 * t + 1.0)
    return (x + 0.01 * torch.randn(n, generator=g, dtype=torch.float64)).float()


def lengths_for(n_fft, hop, frames_per_tile):
    F = frames_per_tile
    wanted = [n_fft // 2 + 1, 3 * hop - 1, 3 * hop, F * hop - 1, F * hop, F * hop + 1, (2 * F + 3) * hop + 7]
    return [max(n, n_fft // 2 + 1) for n in wanted]   # nothing below the shortest legal length
