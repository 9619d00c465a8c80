"""The log-mel spectrogram front end on the device (csrc/melspec.hip, phoneme_recognition/features.py) against the float64 oracle
of tests/melspec_fp64.py, and the acoustic recogniser's data path and entry points on top of it.

Tolerance of every parity check: the kernel's largest error against the fp64 oracle is at most 4 x the largest error of the
stock fp32 path (torch.stft, matmul and log in float32 on the CPU) against the same oracle, both taken on the same inputs:
absolute error for the log-mel, max|a - b| / max|b| for the power.  Both are fp32 pipelines of the same length that differ in
summation order only; on the CPU torch's fp32 path and an independent fp32 pipeline lay within 0.4 - 1.9 x of each other.  Every
parity test first asserts that the oracle's smallest mel power is at least 50 x the clip value, so that no entry lies near the
clip, where the logarithm would amplify rounding without bound."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import yaml

import melspec_fp64 as M
from conftest import ROOT, WORST

pytestmark = pytest.mark.gpu

LOG_CLIP = torch.log(torch.tensor(M.CLIP))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def _features():
    from artspeech_amd.phoneme_recognition import features
    return features


@functools.lru_cache(maxsize=None)
def parity_case(cfg):
    """(lengths, signals, fp64 power per row, stock fp32 power per row) of one configuration; computed once on the CPU"""
    n_fft, win, hop, n_mels = cfg
    lengths = M.lengths_for(n_fft, hop, _features().FRAMES_PER_TILE)
    signals = [M.test_signal(n, seed=100 + i) for i, n in enumerate(lengths)]
    p64 = [M.mel_power(x, n_fft, win, hop, n_mels, torch.float64) for x in signals]
    p32 = [M.mel_power(x, n_fft, win, hop, n_mels, torch.float32) for x in signals]
    return lengths, signals, p64, p32


def nan_pitched_batch(signals, dev, extra=13):
    """the signals as rows of a buffer wider than the longest, NaN behind every row's samples: (view (B, n_max), buffer)"""
    n_max = max(len(x) for x in signals)
    buf = torch.full((len(signals), n_max + extra), float("nan"))
    for b, x in enumerate(signals):
        buf[b, :len(x)] = x
    buf = buf.to(dev)
    return buf[:, :n_max], buf


def assert_far_from_clip(p64):
    smallest = min(float(p.min()) for p in p64)
    assert smallest >= 50 * M.CLIP, f"the oracle's smallest mel power {smallest:.3e} lies within 50 x of the clip {M.CLIP}"


def log_errors(got_rows, p64, p32):
    """(kernel's, stock fp32's) largest absolute log-mel error against the fp64 oracle"""
    ref = [torch.log(torch.clamp(p, min=M.CLIP)) for p in p64]
    stock = [torch.log(torch.clamp(p, min=M.CLIP)) for p in p32]
    err = max(float((g.double() - r).abs().max()) for g, r in zip(got_rows, ref))
    err32 = max(float((s.double() - r).abs().max()) for s, r in zip(stock, ref))
    return err, err32


def power_errors(got_rows, p64, p32):
    err = max(float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(got_rows, p64))
    err32 = max(float((s.double() - r).abs().max() / r.abs().max()) for s, r in zip(p32, p64))
    return err, err32


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("cfg", M.CONFIGS, ids=lambda c: "x".join(map(str, c)))
def test_log_mel_and_power_match_the_fp64_oracle(cfg, channels, dev):
    from artspeech_amd import _lib
    n_fft, win, hop, n_mels = cfg
    lengths, signals, p64, p32 = parity_case(cfg)
    assert_far_from_clip(p64)
    ms = _features().MelSpectrogram(M.SAMPLE_RATE, n_fft, win, hop, n_mels)
    waves, _ = nan_pitched_batch(signals, dev)
    feats, feat_lengths = ms.log_mel_batch(waves, lengths, channels=channels)
    T = [1 + n // hop for n in lengths]
    assert feat_lengths.tolist() == T and feat_lengths.dtype == torch.int64 and not feat_lengths.is_cuda
    assert feats.shape == (len(lengths), channels, n_mels, max(T)) and feats.dtype == torch.float32 and feats.is_cuda
    feats = feats.cpu()
    assert not torch.isnan(feats).any(), "NaN in the output: something read past a row's samples"
    for b, Tb in enumerate(T):
        assert (feats[b, :, :, Tb:] == -1.0).all(), f"row {b}: padding is not exactly -1"
        if channels == 2:
            assert torch.equal(feats[b, 0], feats[b, 1]), f"row {b}: the two planes differ"
    err, err32 = log_errors([feats[b, 0, :, :Tb] for b, Tb in enumerate(T)], p64, p32)
    print(f"log-mel {cfg} channels {channels}: kernel max abs err {err:.3e}, stock fp32 {err32:.3e}, ratio {err / err32:.2f}")
    WORST[f"melspec log {cfg} / stock fp32"] = err / err32
    assert err <= 4 * err32, f"log-mel error {err:.3e} > 4 x the stock fp32 path's {err32:.3e}"

    # the power (clip <= 0) through the C ABI, with the lengths the kernel reports and another padding value
    window, fbanks = ms._device_tables(dev)
    n_dev = torch.tensor(lengths, dtype=torch.int64, device=dev)
    power = torch.empty(len(lengths), channels, n_mels, max(T), device=dev)
    lengths_out = torch.full((len(lengths),), -7, dtype=torch.int64, device=dev)
    _lib.call("as_melspec_fwd", waves, waves.stride(0), n_dev, len(lengths), n_fft, hop, window, fbanks, n_mels, 0.0, channels, 0.25,
              power, max(T), lengths_out)
    assert lengths_out.tolist() == T
    power = power.cpu()
    for b, Tb in enumerate(T):
        assert (power[b, :, :, Tb:] == 0.25).all()
        assert torch.equal(power[b, 0], power[b, -1])
    err, err32 = power_errors([power[b, 0, :, :Tb] for b, Tb in enumerate(T)], p64, p32)
    print(f"power {cfg} channels {channels}: kernel rel err {err:.3e}, stock fp32 {err32:.3e}, ratio {err / err32:.2f}")
    WORST[f"melspec power {cfg} / stock fp32"] = err / err32
    assert err <= 4 * err32, f"power error {err:.3e} > 4 x the stock fp32 path's {err32:.3e}"


def test_forward_returns_the_power_of_equally_long_signals(dev):
    n_fft, win, hop, n_mels = cfg = M.CONFIGS[1]
    n = 5 * hop + 3
    signals = [M.test_signal(n, seed=7 + i) for i in range(6)]
    p64 = [M.mel_power(x, *cfg, torch.float64) for x in signals]
    p32 = [M.mel_power(x, *cfg, torch.float32) for x in signals]
    assert_far_from_clip(p64)
    ms = _features().MelSpectrogram(M.SAMPLE_RATE, n_fft, win, hop, n_mels)
    out = ms(torch.stack(signals).reshape(2, 3, n).to(dev))
    assert out.shape == (2, 3, n_mels, 1 + n // hop)
    err, err32 = power_errors(list(out.cpu().reshape(6, n_mels, -1)), p64, p32)
    assert err <= 4 * err32, (err, err32)
    from artspeech_amd.phoneme_recognition.features import dynamic_range_compression
    logged, _ = ms.log_mel_batch(torch.stack(signals).to(dev), [n] * 6, channels=1)
    err, err32 = log_errors(list(dynamic_range_compression(out).cpu().reshape(6, n_mels, -1)), p64, p32)
    assert err <= 4 * err32, (err, err32)
    err, err32 = log_errors(list(logged.cpu()[:, 0]), p64, p32)
    assert err <= 4 * err32, (err, err32)


def test_silence_is_exactly_log_clip(dev):
    n_fft, win, hop, n_mels = M.CONFIGS[1]
    ms = _features().MelSpectrogram(M.SAMPLE_RATE, n_fft, win, hop, n_mels)
    n = 40 * hop
    quiet_from, quiet_to = 10 * hop, 30 * hop
    x = M.test_signal(n, seed=3)
    x[quiet_from:quiet_to] = 0.0
    waves = torch.stack([torch.zeros(n), x, torch.zeros(n)]).to(dev)
    lengths = [n, n, 17 * hop + 5]
    feats, T = ms.log_mel_batch(waves, lengths)
    feats = feats.cpu()
    for b in (0, 2):
        assert (feats[b, :, :, :T[b]] == LOG_CLIP).all(), "silence is not exactly log(clip)"
    assert (feats[2, :, :, T[2]:] == -1).all()
    # frame t reads the samples [t hop - n_fft / 2, t hop + n_fft / 2): all zeros inside the quiet stretch
    t = torch.arange(T[1])
    only_zeros = (t * hop - n_fft // 2 >= quiet_from) & (t * hop + n_fft // 2 <= quiet_to)
    assert int(only_zeros.sum()) >= 10
    assert (feats[1][:, :, only_zeros] == LOG_CLIP).all()
    assert (feats[1][:, :, :5] > LOG_CLIP).all() and (feats[1][:, :, -5:] > LOG_CLIP).all()


def test_nan_samples_surface_as_nan(dev):
    n_fft, win, hop, n_mels = M.CONFIGS[1]
    ms = _features().MelSpectrogram(M.SAMPLE_RATE, n_fft, win, hop, n_mels)
    n = 40 * hop
    x = M.test_signal(n, seed=5)
    x[20 * hop] = float("nan")
    feats, T = ms.log_mel_batch(torch.stack([x, M.test_signal(n, seed=6)]).to(dev), [n, n])
    feats = feats.cpu()
    t = torch.arange(int(T[0]))
    reads_it = (t * hop - n_fft // 2 <= 20 * hop) & (20 * hop < t * hop + n_fft // 2)
    assert torch.isnan(feats[0][:, :, reads_it]).all(), "a NaN sample is hidden by the clip (torch.clamp propagates it)"
    assert torch.isfinite(feats[0][:, :, ~reads_it]).all() and torch.isfinite(feats[1]).all()


def test_dense_filterbank_takes_the_unstaged_path(dev):
    """a bank denser than the staged weight list holds (here every weight non-zero) is read from memory: the C ABI against the
    fp64 power spectrum times the same bank, by the rule of the parity tests"""
    from artspeech_amd import _lib
    n_fft, win, hop, n_mels = M.CONFIGS[1]
    n_freqs = n_fft // 2 + 1
    g = torch.Generator().manual_seed(11)
    bank = 0.25 + torch.rand(n_freqs, n_mels, generator=g)
    assert int((bank != 0).sum()) > 2 * n_freqs + 256, "the bank must not fit the staged list"
    lengths = M.lengths_for(n_fft, hop, _features().FRAMES_PER_TILE)[-3:]
    signals = [M.test_signal(n, seed=40 + i) for i, n in enumerate(lengths)]

    def power(x, dtype):
        spec = torch.stft(x.to(dtype), n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=dtype),
                          center=True, pad_mode="reflect", return_complex=True)
        return torch.matmul(spec.abs().pow(2).transpose(0, 1), bank.to(dtype)).transpose(0, 1)

    p64, p32 = [power(x, torch.float64) for x in signals], [power(x, torch.float32) for x in signals]
    ms = _features().MelSpectrogram(M.SAMPLE_RATE, n_fft, win, hop, n_mels)
    window, _ = ms._device_tables(dev)
    waves, _ = nan_pitched_batch(signals, dev)
    T = [1 + n // hop for n in lengths]
    out = torch.empty(len(lengths), 1, n_mels, max(T), device=dev)
    n_dev, bank_dev = torch.tensor(lengths, dtype=torch.int64, device=dev), bank.to(dev)   # (held: bare pointers below)
    _lib.call("as_melspec_fwd", waves, waves.stride(0), n_dev, len(lengths), n_fft, hop, window, bank_dev, n_mels, 0.0, 1, -1.0, out,
              max(T), None)
    out = out.cpu()
    err, err32 = power_errors([out[b, 0, :, :Tb] for b, Tb in enumerate(T)], p64, p32)
    print(f"dense bank: kernel rel err {err:.3e}, stock fp32 {err32:.3e}")
    assert err <= 4 * err32, (err, err32)
    assert all((out[b, 0, :, Tb:] == -1).all() for b, Tb in enumerate(T))


def test_repeats_and_rows_alone_are_bit_identical(dev):
    cfg = M.CONFIGS[2]
    n_fft, win, hop, n_mels = cfg
    lengths, signals, _, _ = parity_case(cfg)
    ms = _features().MelSpectrogram(M.SAMPLE_RATE, n_fft, win, hop, n_mels)
    waves, _ = nan_pitched_batch(signals, dev)
    first, T = ms.log_mel_batch(waves, lengths)
    second, _ = ms.log_mel_batch(waves, lengths)
    assert torch.equal(first, second)
    for b, n in enumerate(lengths):
        alone, Tb = ms.log_mel_batch(signals[b][None].to(dev), [n])
        assert int(Tb[0]) == int(T[b]) and torch.equal(alone[0], first[b, :, :, :int(T[b])]), f"row {b} alone differs from row {b} in the batch"


def test_unsupported_shapes_and_short_signals_are_refused(dev):
    F = _features()
    x = M.test_signal(4096, seed=1)[None].to(dev)
    with pytest.raises(RuntimeError, match="n_fft"):
        F.MelSpectrogram(M.SAMPLE_RATE, 1000, 1000, 250, 20).log_mel_batch(x, [4096])
    with pytest.raises(RuntimeError, match="n_mels"):
        F.MelSpectrogram(M.SAMPLE_RATE, 1024, 1024, 256, 129).log_mel_batch(x, [4096])
    ms = F.MelSpectrogram(M.SAMPLE_RATE, 1024, 1024, 256, 80)
    with pytest.raises(RuntimeError, match="channels"):
        ms.log_mel_batch(x, [4096], channels=3)
    for n in (512, 100):   # n <= n_fft / 2: no reflection
        with pytest.raises(ValueError, match="reflect"):
            ms.log_mel_batch(x, [n])
        with pytest.raises(ValueError, match="reflect"):
            ms(x[:, :n])
    with pytest.raises(ValueError, match="exceeds"):
        ms.log_mel_batch(x, [4097])
    feats, T = ms.log_mel_batch(x, [513])   # the shortest legal signal
    assert T.tolist() == [3] and feats.shape == (1, 2, 80, 3)


# ------------------------------------------------------------------------------------------------------------- data path
SMALL_MEL = dict(sample_rate=16000, n_fft=256, win_length=256, hop_length=64, n_mels=8)


def test_acoustic_collate_fn_matches_the_references_layout(dev):
    import train_phoneme_recognition as T
    from artspeech_amd.phoneme_recognition.datasets import SyntheticAcousticRecognitionDataset, acoustic_collate_fn
    vocab = T.build_vocabulary(None, T.Criterion.CTC)
    ds = SyntheticAcousticRecognitionDataset(5, vocab, min_seconds=0.3, max_seconds=0.6, noise=0.05, voiced_tokens=["ph00", "ph01"], seed=4)
    items = [ds[i] for i in range(5)]
    ms = _features().MelSpectrogram(**SMALL_MEL)
    batch = acoustic_collate_fn(items, ms, device=dev)
    # collate_fn on waveform items that carry their transform is the same launch (what the entry scripts' loaders call)
    from artspeech_amd.phoneme_recognition import Feature
    from artspeech_amd.phoneme_recognition.datasets import collate_fn
    ds.melspectrogram = ms
    through = collate_fn([ds[i] for i in range(5)], [Feature.MELSPEC])
    assert set(through) == set(batch) and all(torch.equal(through[k].cpu(), batch[k].cpu()) for k in batch)
    # with a vocabulary the tokens come from the names by the reference's rule, for items without token ids too
    bare = [{k: v for k, v in it.items() if k != "phoneme_tokens"} for it in items]
    named = acoustic_collate_fn(bare, ms, device=dev, vocabulary=vocab)
    assert all(torch.equal(named[k].cpu(), batch[k].cpu()) for k in batch)
    unknown = [dict(bare[0], phonemes_with_time=[("zz", s, e) for _, s, e in bare[0]["phonemes_with_time"]])]
    assert set(acoustic_collate_fn(unknown, ms, device=dev, vocabulary=vocab)["acoustic_target"][0, :-1].tolist()) == {vocab["<unk>"]}
    assert set(batch) == {"melspec", "melspec_length", "acoustic_target", "acoustic_target_length", "articulatory_target",
                          "articulatory_target_length", "voicing", "ctc_target", "ctc_target_length"}
    hop, n_mels = SMALL_MEL["hop_length"], SMALL_MEL["n_mels"]
    L = [1 + it["waveform_length"] // hop for it in items]
    assert batch["melspec"].is_cuda and batch["melspec"].dtype == torch.float32 and batch["melspec"].shape == (5, 2, n_mels, max(L))
    for key in ("melspec_length", "acoustic_target_length", "articulatory_target_length", "ctc_target_length", "acoustic_target",
                "articulatory_target", "ctc_target"):
        assert batch[key].dtype == torch.int64 and not batch[key].is_cuda, key
    assert batch["voicing"].dtype == torch.float32
    assert batch["melspec_length"].tolist() == L == batch["acoustic_target_length"].tolist()
    assert batch["acoustic_target"].shape == (5, max(L))
    mel = batch["melspec"].cpu()
    cfg = (SMALL_MEL["n_fft"], SMALL_MEL["win_length"], hop, n_mels)
    p64 = [M.mel_power(it["waveform"], *cfg, torch.float64) for it in items]
    p32 = [M.mel_power(it["waveform"], *cfg, torch.float32) for it in items]
    assert_far_from_clip(p64)
    err, err32 = log_errors([mel[b, 0, :, :L[b]] for b in range(5)], p64, p32)
    assert err <= 4 * err32, (err, err32)
    for b, it in enumerate(items):
        assert (mel[b, :, :, L[b]:] == -1).all() and torch.equal(mel[b, 0], mel[b, 1])
        want = [0] * L[b]   # the reference's rule with plain ints
        for (name, start, end) in it["phonemes_with_time"]:
            for i in range(int((start * L[b]) / it["audio_duration"]), int((end * L[b]) / it["audio_duration"])):
                want[i] = vocab[name]
        assert batch["acoustic_target"][b, :L[b]].tolist() == want and (batch["acoustic_target"][b, L[b]:] == -1).all()
        assert min(want[:-1]) >= 2, "the intervals cover the utterance: no frame before the last keeps the initial zero"
        for key in ("articulatory_target", "ctc_target", "voicing"):
            n = len(it[key])
            assert torch.equal(batch[key][b, :n], it[key]) and (batch[key][b, n:] == -1).all(), key
        assert int(batch["ctc_target_length"][b]) == len(it["ctc_target"])
        assert int(batch["articulatory_target_length"][b]) == len(it["articulatory_target"])


def test_acoustic_recogniser_trains_and_tests_end_to_end(dev, tmp_path):
    import test_phoneme_recognition as TE
    import train_phoneme_recognition as T
    with open(os.path.join(ROOT, "configs", "train_recognizer_acoustic_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    model = dict(in_channels=2, num_residual_layers=1, num_rnn_layers=1, rnn_hidden_size=16, num_features=20, dropout=0.1)
    mel = {"n_fft": 256, "win_length": 256, "hop_length": 64, "n_mels": 20}
    cfg.update(num_epochs=2, train_seq_dict={"num_sentences": 8}, valid_seq_dict={"num_sentences": 4}, test_seq_dict={"num_sentences": 4},
               synthetic={"min_seconds": 0.3, "max_seconds": 0.6}, melspec=mel, model_params=model, results_dir=str(tmp_path / "train"))
    torch.manual_seed(0)
    out = T.main(**cfg)
    assert len(out["history"]) == 2
    for epoch in out["history"]:
        assert np.isfinite(epoch["train"]["loss"]) and np.isfinite(epoch["valid"]["loss"]), epoch
    for name in ("best_model.pt", "last_model.pt", "info_test.json", "substitution_matrix.npy", "confusion_matrix.npy"):
        assert os.path.exists(tmp_path / "train" / name), name
    with open(tmp_path / "train" / "info_test.json") as f:
        info = json.load(f)
    assert np.isfinite(info["loss"]) and np.isfinite(info["edit_distance"])
    confusion = np.load(tmp_path / "train" / "confusion_matrix.npy")
    assert confusion.ndim == 2 and confusion.shape[0] == confusion.shape[1] and np.isfinite(confusion).all()

    with open(os.path.join(ROOT, "configs", "test_recognizer_acoustic_synthetic.yaml")) as f:
        tcfg = yaml.safe_load(f)
    tcfg.update(seq_dict={"num_sentences": 4}, synthetic={"min_seconds": 0.3, "max_seconds": 0.6, "melspec": mel}, model_params=model,
                state_dict_filepath=str(tmp_path / "train" / "best_model.pt"), save_dir=str(tmp_path / "test"))
    info = TE.main(**tcfg)
    assert np.isfinite(info["edit_distance"]) and np.isfinite(info["word_info_lost"])
    for name in ("info_test.json", "substitution_matrix.npy", "confusion_matrix.npy"):
        assert os.path.exists(tmp_path / "test" / name), name
