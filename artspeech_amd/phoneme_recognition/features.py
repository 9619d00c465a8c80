"""The speech-signal feature of the acoustic recogniser (reference ``phoneme_recognition/datasets.py``:84-92, 123-132, 47-48): a
mel spectrogram with torchaudio's ``transforms.MelSpectrogram`` keywords and defaults, computed on the device by
``as_melspec_fwd`` (csrc/melspec.hip).  ``MelSpectrogram.forward`` returns the power mel spectrogram of one tensor of equally long
signals; ``MelSpectrogram.log_mel_batch`` is the launch the data path uses: padded waveforms of different lengths in, the collated
``(B, channels, n_mels, T_max)`` log-mel batch out.  The window and the filterbank are built once per transform on the host in
float64 and rounded to float32.  torchaudio is not a dependency; the formulas are written from its documentation (periodic Hann
window, centred reflect-padded frames, power 2, ``melscale_fbanks(norm=None, mel_scale="htk")``) and parity with it is unpinned.
Ahead of it, ``Resample`` / ``resample`` (torchaudio's names and keywords) bring recordings at another rate to the model's on the
device: ``as_resample_fwd`` (csrc/resample.hip), the first step of the reference's ``load_melspec`` (:124-126)."""
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


# ------------------------------------------------------------------------------------------------------------------ resampling
# The first step of the reference's load_melspec (datasets.py:124-126): F.resample(audio, orig_freq, new_freq) when a recording's
# rate is not the model's.  torchaudio's polyphase windowed-sinc resampler, written from its documentation, on the device by
# as_resample_fwd (csrc/resample.hip); parity with torchaudio is unpinned, like the mel spectrogram's.
MAX_PHASES, MAX_BAND, MAX_ROW = 1024, 512, 0x3fff0000   # AS_RESAMPLE_MAX_* of the header
KAISER_BETA = 14.769656459379492
BAND_THRESHOLD = 1e-20   # a tap of the dense filter at or below this magnitude lies outside its phase's band


def sinc_resample_kernel(orig_freq, new_freq, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, beta=None):
    """(h (n, 2 width + o) float64, width) of the documentation's filter for the integer rates: o = orig / gcd, n = new / gcd,
    base = min(o, n) rolloff, width = ceil(lowpass_filter_width o / base), and for phase i and tap k
    t = clamp((-i / n + (k - width) / o) base, +-lowpass_filter_width), h[i][k] = sinc(pi t) window(t) base / o."""
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq < 1 or new_freq < 1:
        raise ValueError(f"Resample: the rates must be positive integers, got {orig_freq} and {new_freq}")
    if resampling_method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
        raise ValueError(f"Resample: resampling_method {resampling_method!r} is neither sinc_interp_hann nor sinc_interp_kaiser")
    if lowpass_filter_width < 1 or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"Resample: lowpass_filter_width {lowpass_filter_width} must be positive and rolloff {rolloff} in (0, 1]")
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    k = torch.arange(-width, width + o, dtype=torch.float64)
    i = torch.arange(n, dtype=torch.float64)
    t = ((-i[:, None] / n + k[None, :] / o) * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lowpass_filter_width / 2.0) ** 2
    else:
        b = torch.tensor(KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
        window = torch.special.i0(b * torch.sqrt(1.0 - (t / lowpass_filter_width) ** 2)) / torch.special.i0(b)
    tp = t * math.pi
    sinc = torch.where(tp == 0, torch.ones_like(tp), torch.sin(tp) / torch.where(tp == 0, torch.ones_like(tp), tp))
    return sinc * window * (base / o), width


def banded_table(h):
    """(first (n,) int32, coef (band, n) float64) of the dense filter h (n, K): phase i's band runs from its first to its last tap
    above BAND_THRESHOLD, every phase stores `band` = the longest such run taps from first[i] on (moved left where the run would
    pass K), and coef[q][i] = h[i][first[i] + q] -- the dense values themselves, tap-major."""
    n, K = h.shape
    live = h.abs() > BAND_THRESHOLD
    if not bool(live.any(dim=1).all()):
        raise ValueError("Resample: a phase of the filter has no tap above the band threshold")
    taps = torch.arange(K)
    lo = torch.where(live, taps, K).min(dim=1).values
    hi = torch.where(live, taps, -1).max(dim=1).values
    band = int((hi - lo).max()) + 1
    first = torch.minimum(lo, torch.tensor(K - band))
    coef = h.gather(1, first[:, None] + torch.arange(band)[None, :]).t().contiguous()
    return first.to(torch.int32), coef


def resampled_length(n_samples, o, n):
    """ceil(n L / o) in integers (an int or an int64 tensor); torchaudio takes the ceiling of a float32 product instead"""
    return (n * n_samples + o - 1) // o


class Resample:
    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99,
                 beta=None):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.resampling_method, self.lowpass_filter_width, self.rolloff, self.beta = resampling_method, lowpass_filter_width, rolloff, beta
        h, self.width = sinc_resample_kernel(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta)
        g = math.gcd(self.orig_freq, self.new_freq)
        self.o, self.n = self.orig_freq // g, self.new_freq // g
        self.first, coef = banded_table(h)
        self.coef = coef.float().contiguous()          # (band, n)
        self.band = self.coef.shape[0]
        lead = self.first.long() - self.width - torch.arange(self.n) * self.o // self.n
        self.lead_min, self.lead_max = int(lead.min()), int(lead.max())
        self._tables = {}   # device -> (coef, first)

    @property
    def tile(self):
        """outputs one workgroup computes at this ratio (the host's choice, as_resample_tile); 0: the ratio is not supported"""
        return _lib.call("as_resample_tile", self.o, self.n, self.band, self.lead_max - self.lead_min)

    @property
    def tile_inputs(self):
        """input samples that a full tile of outputs covers: ceil(tile o / n)"""
        return -(-self.tile * self.o // self.n)

    def target_length(self, n_samples):
        return resampled_length(n_samples, self.o, self.n)

    def _device_tables(self, device):
        if device not in self._tables:
            self._tables[device] = (self.coef.to(device), self.first.to(device))
        return self._tables[device]

    def _launch(self, waveforms, lengths_host, pad_value, out=None):
        _lib.require_gpu(waveforms, "Resample: waveform")
        if waveforms.dtype not in (torch.float32, torch.int16) or waveforms.dim() != 2 or (waveforms.shape[1] > 1 and waveforms.stride(1) != 1):
            raise ValueError("Resample: waveforms must be (B, n) float32 or int16 with unit sample stride")
        B, n_max = waveforms.shape
        lengths_host = torch.as_tensor(lengths_host, dtype=torch.int64).reshape(-1).cpu()
        if lengths_host.numel() != B:
            raise ValueError(f"Resample: {lengths_host.numel()} lengths for {B} waveforms")
        if B == 0 or int(lengths_host.min()) < 1:
            raise ValueError("Resample: every waveform needs at least one sample")
        if int(lengths_host.max()) > n_max:
            raise ValueError(f"Resample: length {int(lengths_host.max())} exceeds the {n_max} samples of a row")
        pitch = waveforms.stride(0) if B > 1 else n_max
        if pitch < n_max:
            raise ValueError("Resample: overlapping waveform rows")
        new_lengths = self.target_length(lengths_host)
        if out is None:
            out = torch.empty(B, int(new_lengths.max()), dtype=torch.float32, device=waveforms.device)
        elif (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.device != waveforms.device
              or out.shape[1] < int(new_lengths.max()) or (out.shape[1] > 1 and out.stride(1) != 1) or (B > 1 and out.stride(0) < out.shape[1])):
            raise ValueError(f"Resample: out must be ({B}, >= {int(new_lengths.max())}) float32 rows on the waveforms' device")
        m_max = out.shape[1]
        coef, first = self._device_tables(waveforms.device)
        # the lengths travel through pinned memory without blocking, as in MelSpectrogram._launch
        n_samples = lengths_host.pin_memory().to(waveforms.device, non_blocking=True)
        _lib.call("as_resample_fwd", waveforms, int(waveforms.dtype == torch.int16), pitch, n_samples, B, self.o, self.n, coef, first,
                  self.band, self.width, self.lead_min, self.lead_max, pad_value, out, out.stride(0) if B > 1 else m_max, m_max, None)
        return out, new_lengths

    def forward(self, waveform):
        """(..., ceil(n new / orig)) float32 of a device tensor (..., n), float32 or int16 (read as value / 32768); the input
        itself, without a launch, when the rates are equal"""
        _lib.require_gpu(waveform, "Resample: waveform")
        if self.orig_freq == self.new_freq:
            return waveform
        lead, n = waveform.shape[:-1], waveform.shape[-1]
        flat = waveform.reshape(-1, n)
        flat = _lib.contiguous(flat if flat.dtype == torch.int16 else flat.float())
        out, _ = self._launch(flat, torch.full((flat.shape[0],), n, dtype=torch.int64), 0.0)
        return out.reshape(*lead, out.shape[-1])

    __call__ = forward

    def resample_batch(self, waveforms, lengths, pad_value=0.0, out=None):
        """(rows (B, m_max) float32 on the device, new lengths (B,) int64 on the host) of the padded waveforms (B, n_max) on the
        device, float32 or int16: row b holds its ceil(lengths[b] new / orig) samples and pad_value behind them.  One launch on the
        current stream, no synchronisation; `out` (B, >= the longest new length) receives the rows instead of a new tensor, so
        that several rates fill one buffer.  Equal rates: the arguments come back as they are, without a launch."""
        if self.orig_freq == self.new_freq:
            if out is not None:
                raise ValueError("Resample.resample_batch: equal rates launch nothing and fill no `out`")
            _lib.require_gpu(waveforms, "Resample: waveform")
            return waveforms, torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).cpu()
        return self._launch(waveforms, lengths, float(pad_value), out)


_RESAMPLERS = {}


def resampler(orig_freq, new_freq, **kw):
    """the Resample of these rates and keywords, built once per process (its table lives on the device it was used on)"""
    key = (int(orig_freq), int(new_freq), tuple(sorted(kw.items())))
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = Resample(orig_freq, new_freq, **kw)
    return _RESAMPLERS[key]


def resample(waveform, orig_freq, new_freq, **kw):
    """torchaudio.functional.resample's call: Resample(orig_freq, new_freq, **kw)(waveform), the transform cached per keywords"""
    return resampler(orig_freq, new_freq, **kw)(waveform)
