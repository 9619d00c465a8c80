"""The speech-signal feature of the acoustic recogniser (reference ``phoneme_recognition/datasets.py``:84-92, 123-132, 47-48): a
mel spectrogram with torchaudio's ``transforms.MelSpectrogram`` keywords and defaults, computed on the device by
``as_melspec_fwd`` (csrc/melspec.hip).  ``MelSpectrogram.forward`` returns the power mel spectrogram of one tensor of equally long
signals; ``MelSpectrogram.log_mel_batch`` is the launch the data path uses: padded waveforms of different lengths in, the collated
``(B, channels, n_mels, T_max)`` log-mel batch out.  The window and the filterbank are built once per transform on the host in
float64 and rounded to float32.  torchaudio is not a dependency; the formulas are written from its documentation (periodic Hann
window, centred reflect-padded frames, power 2, ``melscale_fbanks(norm=None, mel_scale="htk")``) and parity with it is unpinned."""
import math

import torch

from .. import _lib

FRAMES_PER_TILE = 16   # MEL_FRAMES_PER_TILE of csrc/melspec.hip: frames one workgroup computes
MIN_N_FFT, MAX_N_FFT, MAX_N_MELS = 64, 2048, 128


def _hz_to_mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate):
    """(n_freqs, n_mels) float64 triangular filters: bin k stands at linspace(0, sample_rate // 2, n_freqs)[k], the n_mels + 2
    corner frequencies are evenly spaced on the HTK mel scale between f_min and f_max, no area normalisation."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(_hz_to_mel(f_min), _hz_to_mel(f_max), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (torch.pow(10.0, m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]                        # (n_mels + 1,)
    slopes = f_pts[None, :] - all_freqs[:, None]           # (n_freqs, n_mels + 2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


def frame_count(n_samples, hop_length):
    """frames of a centred STFT: 1 + n // hop"""
    return 1 + n_samples // hop_length


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


class MelSpectrogram:
    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, n_mels=128, f_min=0.0, f_max=None):
        self.sample_rate, self.n_fft, self.n_mels = sample_rate, n_fft, n_mels
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        if not 0 < self.win_length <= n_fft:
            raise ValueError(f"MelSpectrogram: win_length {self.win_length} must lie in (0, n_fft = {n_fft}]")
        if self.hop_length < 1:
            raise ValueError(f"MelSpectrogram: hop_length {self.hop_length} must be positive")
        i = torch.arange(self.win_length, dtype=torch.float64)
        window = torch.zeros(n_fft, dtype=torch.float64)
        left = (n_fft - self.win_length) // 2
        window[left:left + self.win_length] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * i / self.win_length)
        self.window = window.float()
        self.fbanks = mel_filterbank(n_fft // 2 + 1, self.f_min, self.f_max, n_mels, sample_rate).float().contiguous()
        self._tables = {}   # device -> (window, fbanks)

    def _device_tables(self, device):
        if device not in self._tables:
            self._tables[device] = (self.window.to(device), self.fbanks.to(device))
        return self._tables[device]

    def _launch(self, waveforms, lengths_host, clip, channels, pad_value):
        _lib.require_gpu(waveforms, "MelSpectrogram: waveform")
        if waveforms.dtype != torch.float32 or waveforms.dim() != 2 or (waveforms.shape[1] > 1 and waveforms.stride(1) != 1):
            raise ValueError("MelSpectrogram: waveforms must be (B, n) float32 with unit sample stride")
        B, n_max = waveforms.shape
        lengths_host = torch.as_tensor(lengths_host, dtype=torch.int64).reshape(-1).cpu()
        if lengths_host.numel() != B:
            raise ValueError(f"MelSpectrogram: {lengths_host.numel()} lengths for {B} waveforms")
        shortest, longest = int(lengths_host.min()), int(lengths_host.max())
        if shortest <= self.n_fft // 2:
            raise ValueError(f"MelSpectrogram: a signal of {shortest} samples cannot be reflect-padded by n_fft / 2 = "
                             f"{self.n_fft // 2}; it needs more than that many samples")
        if longest > n_max:
            raise ValueError(f"MelSpectrogram: length {longest} exceeds the {n_max} samples of a row")
        pitch = waveforms.stride(0) if B > 1 else max(n_max, 1)
        if pitch < n_max:
            raise ValueError("MelSpectrogram: overlapping waveform rows")
        window, fbanks = self._device_tables(waveforms.device)
        T_max = frame_count(longest, self.hop_length)
        out = torch.empty(B, channels, self.n_mels, T_max, dtype=torch.float32, device=waveforms.device)
        # the lengths travel through pinned memory without blocking: a pageable copy would wait for the stream to drain on every call
        n_samples = lengths_host.pin_memory().to(waveforms.device, non_blocking=True)
        _lib.call("as_melspec_fwd", waveforms, pitch, n_samples, B, self.n_fft, self.hop_length, window, fbanks, self.n_mels, clip,
                  channels, pad_value, out, T_max, None)
        return out, frame_count(lengths_host, self.hop_length)

    def forward(self, waveform):
        """power mel spectrogram (..., n_mels, 1 + n // hop) of a device tensor (..., n)"""
        _lib.require_gpu(waveform, "MelSpectrogram: waveform")
        lead, n = waveform.shape[:-1], waveform.shape[-1]
        flat = _lib.contiguous(waveform.reshape(-1, n).float())
        out, _ = self._launch(flat, torch.full((flat.shape[0],), n, dtype=torch.int64), 0.0, 1, 0.0)
        return out.reshape(*lead, self.n_mels, out.shape[-1])

    __call__ = forward

    def log_mel_batch(self, waveforms, lengths, channels=2, clip_val=1e-5, pad_value=-1.0):
        """(features (B, channels, n_mels, T_max) on the device, feature_lengths (B,) int64 on the host) of the padded waveforms
        (B, n_max) on the device: log(max(mel, clip_val)) in every plane at t < 1 + lengths[b] // hop, pad_value behind it.  One
        launch for the reference's load_melspec + dynamic_range_compression + the feature part of collate_fn."""
        if not clip_val > 0:
            raise ValueError("MelSpectrogram.log_mel_batch: clip_val must be positive (forward() returns the power)")
        return self._launch(waveforms, lengths, float(clip_val), channels, float(pad_value))
