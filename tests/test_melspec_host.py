"""Host-side pieces of the acoustic recogniser's front end (no GPU): the mel filterbank against the restatement of
tests/melspec_fp64.py and its properties, the window, the frame count, the refusals, the synthetic waveform data set, the new
configs and the new entry point of the header."""
import inspect
import os
import re

import pytest
import torch
import yaml

import melspec_fp64 as M
from conftest import ROOT


def _vocab():
    return {"<blank>": 0, "<unk>": 1, **{f"ph{i:02d}": i + 2 for i in range(6)}}


@pytest.mark.parametrize("cfg", M.CONFIGS, ids=lambda c: "x".join(map(str, c)))
def test_filterbank_and_window_equal_the_restatement(cfg):
    from artspeech_amd.phoneme_recognition.features import MelSpectrogram, mel_filterbank
    n_fft, win, hop, n_mels = cfg
    fb = mel_filterbank(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000)
    ref = M.filterbank_fp64(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000)
    assert fb.dtype == torch.float64 and fb.shape == (n_fft // 2 + 1, n_mels)
    assert float((fb - ref).abs().max()) <= 1e-12
    ms = MelSpectrogram(16000, n_fft, win, hop, n_mels)
    assert ms.fbanks.dtype == torch.float32 and torch.equal(ms.fbanks, fb.float())
    assert ms.window.dtype == torch.float32 and ms.window.shape == (n_fft,)
    assert float((ms.window.double() - M.window_fp64(n_fft, win)).abs().max()) <= 1e-7
    left = (n_fft - win) // 2
    assert (ms.window[:left] == 0).all() and (ms.window[left + win:] == 0).all() and ms.window[left + win // 2] == 1.0


def test_filterbank_properties_at_the_thesis_parameters():
    from artspeech_amd.phoneme_recognition.features import mel_filterbank
    fb = mel_filterbank(513, 0.0, 8000.0, 80, 16000)
    assert fb.shape == (513, 80) and (fb >= 0).all() and float(fb.max()) <= 1.0
    assert (fb.sum(dim=0) > 0).all(), "an empty filter at the thesis parameters"
    assert int((fb > 0).sum(dim=1).max()) <= 2, "a bin feeds at most two filters"
    for m in range(80):   # one triangle: a contiguous support, rising to one peak, then falling
        col = fb[:, m]
        nz = torch.nonzero(col).flatten()
        assert int(nz[-1] - nz[0]) + 1 == len(nz), m
        peak = int(col.argmax())
        assert (col[int(nz[0]):peak + 1].diff() >= 0).all() and (col[peak:int(nz[-1]) + 1].diff() <= 0).all(), m
    peaks = fb.argmax(dim=0)
    assert (peaks.diff() > 0).all()


def test_defaults_are_torchaudios_and_the_frame_count():
    from artspeech_amd.phoneme_recognition.features import FRAMES_PER_TILE, MelSpectrogram, frame_count
    ms = MelSpectrogram()
    assert (ms.sample_rate, ms.n_fft, ms.win_length, ms.hop_length, ms.n_mels, ms.f_min, ms.f_max) == (16000, 400, 400, 200, 128, 0.0, 8000.0)
    assert list(inspect.signature(MelSpectrogram.__init__).parameters)[1:] == ["sample_rate", "n_fft", "win_length", "hop_length", "n_mels",
                                                                              "f_min", "f_max"]
    assert MelSpectrogram(n_fft=512, win_length=300).hop_length == 150
    for n, hop in ((513, 256), (767, 256), (768, 256), (64000, 256), (33, 16)):
        x = torch.zeros(n)
        frames = torch.stft(x, 64 if hop == 16 else 1024, hop_length=hop, window=torch.ones(64 if hop == 16 else 1024), center=True,
                            pad_mode="reflect", return_complex=True).shape[-1]
        assert frame_count(n, hop) == frames == 1 + n // hop
    assert frame_count(torch.tensor([512, 513]), 256).tolist() == [3, 3]
    with open(os.path.join(ROOT, "artspeech_amd", "csrc", "melspec.hip")) as f:
        assert int(re.search(r"#define MEL_FRAMES_PER_TILE (\d+)", f.read()).group(1)) == FRAMES_PER_TILE


def test_host_tensors_mean_a_loud_error_not_a_host_path():
    from artspeech_amd.phoneme_recognition.features import MelSpectrogram, dynamic_range_compression
    ms = MelSpectrogram(16000, 1024, 1024, 256, 80)
    with pytest.raises(RuntimeError, match="MI355X"):
        ms(torch.zeros(2, 4000))
    with pytest.raises(RuntimeError, match="MI355X"):
        ms.log_mel_batch(torch.zeros(2, 4000), [4000, 3000])
    x = torch.tensor([0.0, 1e-6, 1e-5, 2.0])
    assert torch.equal(dynamic_range_compression(x), torch.log(torch.tensor([1e-5, 1e-5, 1e-5, 2.0])))
    with pytest.raises(ValueError, match="win_length"):
        MelSpectrogram(n_fft=256, win_length=512)


def test_synthetic_acoustic_data_set_is_seeded_and_has_the_item_keys():
    from artspeech_amd.phoneme_recognition.datasets import SyntheticAcousticRecognitionDataset, acoustic_target
    vocab = _vocab()
    kw = dict(min_seconds=0.3, max_seconds=0.6, voiced_tokens=["ph00"])
    ds, again, other = (SyntheticAcousticRecognitionDataset(4, vocab, seed=s, **kw) for s in (5, 5, 6))
    assert len(ds) == 4
    names = {i: t for t, i in vocab.items()}
    for i in range(4):
        a, b = ds[i], again[i]
        assert set(a) == {"waveform", "waveform_length", "audio_duration", "phonemes_with_time", "phoneme_tokens", "articulatory_target",
                          "articulatory_target_length", "voicing", "ctc_target", "ctc_target_length"}
        assert torch.equal(a["waveform"], b["waveform"]) and a["phonemes_with_time"] == b["phonemes_with_time"]
        assert not torch.equal(a["waveform"][:1000], other[i]["waveform"][:1000])
        n = a["waveform_length"]
        assert a["waveform"].shape == (n,) and a["waveform"].dtype == torch.float32 and 4800 <= n <= 9600
        assert a["audio_duration"] == n / 16000 and float(a["waveform"].abs().max()) < 2.0
        spans = a["phonemes_with_time"]
        assert spans[0][1] == 0.0 and spans[-1][2] == a["audio_duration"]
        assert all(s0[2] == s1[1] for s0, s1 in zip(spans, spans[1:]))                       # back to back
        assert all(0.06 - 1e-9 <= e - s <= 0.2 + 1e-9 for _, s, e in spans[:-1]) and spans[-1][2] - spans[-1][1] <= 0.2 + 1e-9
        tokens = [vocab[name] for name, _, _ in spans]
        assert tokens == a["phoneme_tokens"] and min(tokens) >= 2
        assert torch.equal(a["ctc_target"], torch.unique_consecutive(torch.tensor(tokens))) and a["ctc_target_length"] == len(a["ctc_target"])
        T = a["articulatory_target_length"]
        assert T == int(a["audio_duration"] * 50) == len(a["articulatory_target"]) == len(a["voicing"])
        for f in (0, T // 2, T - 1):   # the token of the frame's centre
            at = (f + 0.5) / 50
            assert names[int(a["articulatory_target"][f])] == next(name for name, s, e in spans if s <= at < e)
        assert torch.equal(a["voicing"], (a["articulatory_target"] == vocab["ph00"]).float())
        target = acoustic_target(spans, tokens, 40, a["audio_duration"])
        assert target.dtype == torch.int64 and target.shape == (40,) and (target[:-1] >= 2).all()
    # the prototypes are shared by the splits: the same token sounds the same
    assert torch.equal(ds.frequencies, other.frequencies) and torch.equal(ds.amplitudes, other.amplitudes)
    assert not torch.equal(ds.frequencies, SyntheticAcousticRecognitionDataset(1, vocab, prototype_seed=1).frequencies)


def test_new_configs_are_main_arguments_and_the_thesis_model():
    import test_phoneme_recognition as TE
    import train_phoneme_recognition as T
    cfgs = {}
    for script, name in ((T, "train_recognizer_acoustic_synthetic.yaml"), (TE, "test_recognizer_acoustic_synthetic.yaml")):
        params = inspect.signature(script.main).parameters
        with open(os.path.join(ROOT, "configs", name)) as f:
            cfg = cfgs[script] = yaml.safe_load(f)
        assert set(cfg) <= set(params), set(cfg) - set(params)
        assert cfg["feature"] == "melspec" and cfg["target"] == "ctc_target" and cfg["plot_target"] == "acoustic_target"
        assert cfg["model_params"] == dict(in_channels=2, num_residual_layers=4, num_rnn_layers=2, rnn_hidden_size=64, num_features=80,
                                           dropout=0.1)
        assert cfg["loss"] == "CTC" and cfg["batch_size"] == 4 and cfg["num_workers"] == 0 and cfg["datadir"] == "synthetic"
    train, test = cfgs[T], cfgs[TE]
    # the trainer takes the transform's keywords as its new trailing keyword; the test script's main() is the parent's, so its
    # config carries them inside `synthetic`, where _make_dataset reads them
    params = inspect.signature(T.main).parameters
    assert list(params)[-1] == "melspec" and params["melspec"].default is None
    reference = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop_length=256, n_mels=80)
    assert train["melspec"] == test["synthetic"]["melspec"] == T.MELSPEC_DEFAULTS == reference
    assert train["loss_params"] == {"zero_infinity": True} and train["logits_large_margins"] == 0.0005
    assert test["state_dict_filepath"] == os.path.join(train["results_dir"], "best_model.pt")


def test_make_dataset_builds_the_waveform_set_with_its_transform():
    import train_phoneme_recognition as T
    from artspeech_amd.phoneme_recognition.datasets import SyntheticAcousticRecognitionDataset, collate_fn
    vocab = _vocab()
    small = {"n_fft": 256, "win_length": 256, "hop_length": 64, "n_mels": 20}
    for synthetic, melspec in (({"min_seconds": 0.3, "max_seconds": 0.6, "melspec": small}, None),
                               ({"min_seconds": 0.3, "max_seconds": 0.6}, small),
                               ({"min_seconds": 0.3, "max_seconds": 0.6, "melspec": {"n_fft": 512}}, small)):
        ds = T._make_dataset("synthetic", "artspeech2", {"num_sentences": 3}, vocab, T.Feature.MELSPEC, None, synthetic, 7, melspec)
        assert isinstance(ds, SyntheticAcousticRecognitionDataset) and len(ds) == 3 and ds.sample_rate == 16000
        ms = ds.melspectrogram
        assert (ms.n_fft, ms.win_length, ms.hop_length, ms.n_mels, ms.sample_rate) == (256, 256, 64, 20, 16000)
        assert ds[0]["melspectrogram"] is ms and 4800 <= ds[0]["waveform_length"] <= 9600
    default = T._make_dataset("synthetic", "artspeech2", {"num_sentences": 1}, vocab, T.Feature.MELSPEC, None, None, 0)
    assert (default.melspectrogram.n_fft, default.melspectrogram.hop_length, default.melspectrogram.n_mels) == (1024, 256, 80)
    with pytest.raises(RuntimeError, match="MI355X"):   # collate_fn launches the transform: there is no host path
        collate_fn([ds[0], ds[1]], [T.Feature.MELSPEC])
    bare = SyntheticAcousticRecognitionDataset(2, vocab, min_seconds=0.3, max_seconds=0.6)
    with pytest.raises(ValueError, match="MelSpectrogram"):
        collate_fn([bare[0], bare[1]], [T.Feature.MELSPEC])
    articulatory = T._make_dataset("synthetic", "artspeech2", {"num_sentences": 2}, vocab, T.Feature.VOCAL_TRACT, None, {"min_len": 6, "max_len": 9}, 0)
    assert "vocal_tract" in articulatory[0]


def test_melspec_with_voicing_or_workers_raises(tmp_path, monkeypatch):
    import train_phoneme_recognition as T
    voicing = tmp_path / "voiced.json"
    voicing.write_text('["ph00"]')
    with open(os.path.join(ROOT, "configs", "train_recognizer_acoustic_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    with pytest.raises(ValueError, match="voicing"):
        T.main(**dict(cfg, voicing_filepath=str(voicing), results_dir=str(tmp_path / "r")))
    assert not os.path.exists(tmp_path / "r")
    with pytest.raises(ValueError, match="voicing"):   # what test_phoneme_recognition.py reaches with a voicing_filepath
        T._make_dataset("synthetic", "artspeech2", {"num_sentences": 2}, _vocab(), T.Feature.MELSPEC, ["ph00"], None, 0)
    with pytest.raises(ValueError, match="num_workers"):
        T.make_collate_fn("synthetic", T.Feature.MELSPEC, 2)
    # and inside a DataLoader worker, which is where test_phoneme_recognition.py's num_workers > 0 would put the launch
    import torch.utils.data
    from artspeech_amd.phoneme_recognition.datasets import collate_fn
    ds = T._make_dataset("synthetic", "artspeech2", {"num_sentences": 2}, _vocab(), T.Feature.MELSPEC, None,
                         {"min_seconds": 0.3, "max_seconds": 0.6}, 0)
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(ValueError, match="num_workers"):
        collate_fn([ds[0], ds[1]], [T.Feature.MELSPEC])


def test_header_declares_and_binding_binds_the_entry_point():
    from artspeech_amd import _lib, build
    with open(os.path.join(ROOT, "include", "artspeech_hip.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint as_melspec_fwd\s*\(", header)
    for site in ("datasets.py:84-92", ":123-132", ":47-48", ":258-260"):
        assert site in text, f"the reference call site {site} is not cited"
    L = _lib.lib()
    assert "as_melspec_fwd" in _lib.PROTOTYPES and hasattr(L, "as_melspec_fwd")
    res, args = _lib.PROTOTYPES["as_melspec_fwd"]
    assert len(args) == 16 and args[-1] is _lib.Stream
    assert build.SOURCES["melspec.hip"] == [] and os.path.exists(os.path.join(build.CSRC, "melspec.hip"))
