"""Host-side pieces of the resampler ahead of the log-mel (no GPU): the banded filter table against the restatement of
tests/resample_fp64.py, the target lengths, the planner under the sanitizers, the refusals, the WAV reader, the manifest data set,
the synthetic data set at a foreign rate, the new configs and the new entry point of the header."""
import inspect
import json
import math
import os
import re
import subprocess
import wave

import numpy as np
import pytest
import torch
import yaml

import resample_fp64 as R
from conftest import ROOT

VARIANTS = [{}, {"lowpass_filter_width": 16}, {"rolloff": 0.9}]


def _vocab():
    return {"<blank>": 0, "<unk>": 1, **{f"ph{i:02d}": i + 2 for i in range(6)}}


def _write_wav(path, samples, rate, width=2):
    """samples (n, channels) int16 (or int32 for 24-bit: the low three bytes are written)"""
    with wave.open(str(path), "wb") as f:
        f.setnchannels(samples.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        if width == 2:
            f.writeframes(samples.astype("<i2").tobytes())
        else:
            f.writeframes(b"".join(int(v).to_bytes(4, "little", signed=True)[:width] for v in samples.reshape(-1)))


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("rates", R.RATIOS, ids=lambda r: f"{r[0]}to{r[1]}")
def test_banded_table_equals_the_restatement_inside_the_band(rates, method):
    from artspeech_amd.phoneme_recognition.features import MAX_BAND, MAX_PHASES, Resample, sinc_resample_kernel
    for kw in VARIANTS:
        h, width = R.dense_table(*rates, method, **kw)
        rs = Resample(*rates, resampling_method=method, **kw)
        o, n = R.ratio(*rates)
        K = 2 * width + o
        assert (rs.o, rs.n, rs.width) == (o, n, width) and h.shape == (n, K)
        own, own_width = sinc_resample_kernel(*rates, method, **kw)
        assert own_width == width and own.dtype == torch.float64 and float((own - h).abs().max()) <= 1e-14
        assert rs.coef.dtype == torch.float32 and rs.coef.shape == (rs.band, n) and rs.coef.is_contiguous()
        assert rs.first.dtype == torch.int32 and rs.first.shape == (n,)
        assert rs.band <= 2 * width + 2 and rs.band <= MAX_BAND and n <= MAX_PHASES
        assert int(rs.first.min()) >= 0 and int(rs.first.max()) + rs.band <= K
        lo, hi = R.band_of(h)
        outside = h.clone()
        for i in range(n):
            a = int(rs.first[i])
            assert a <= int(lo[i]) and int(hi[i]) < a + rs.band, f"phase {i}: the band [{a}, {a + rs.band}) misses a live tap"
            # fp32 of the package's own float64 table, which equals the restatement's to 1e-14: one float32 ulp at the most apart
            band = h[i, a:a + rs.band]
            assert float((rs.coef[:, i].double() - band).abs().max()) <= 2.0 ** -23 * float(band.abs().max())
            assert torch.equal(rs.coef[:, i], own[i, a:a + rs.band].float())
            outside[i, a:a + rs.band] = 0.0
        assert float(outside.abs().max()) <= 1e-20, "a tap outside the band is not negligible"
        lead = rs.first.long() - width - torch.arange(n) * o // n
        assert (rs.lead_min, rs.lead_max) == (int(lead.min()), int(lead.max()))
        assert rs.tile == 1024 and rs.tile_inputs == -(-1024 * o // n)


def test_band_lengths_of_the_usual_rates():
    from artspeech_amd.phoneme_recognition.features import Resample
    for rates, taps, K in (((44100, 16000), (33, 34), 475), ((8000, 16000), (12, 13), 15), ((48000, 16000), (37, 37), 41),
                           ((22050, 16000), (16, 17), 459), ((16000, 44100), (12, 13), 174)):
        h, width = R.dense_table(*rates)
        lo, hi = R.band_of(h)
        assert h.shape[1] == K and (int((hi - lo).min()) + 1, int((hi - lo).max()) + 1) == taps
        assert Resample(*rates).band == taps[1]


def test_target_lengths_follow_the_integer_formula():
    from artspeech_amd.phoneme_recognition.features import Resample, resampled_length
    for rates in R.RATIOS + [(8000, 16000), (16000, 8000), (11025, 16000)]:
        rs = Resample(*rates)
        o, n = R.ratio(*rates)
        lengths = list(range(1, 60)) + [o - 1, o, o + 1, 7 * o + 3, 44100 * 70 + 1, 2 ** 30 - 5]
        want = [-((-n * L) // o) for L in lengths]
        assert [rs.target_length(L) for L in lengths] == want == [math.ceil(n * L / o) if L < 2 ** 20 else w for L, w in zip(lengths, want)]
        got = rs.target_length(torch.tensor(lengths))
        assert got.dtype == torch.int64 and got.tolist() == want == [resampled_length(L, o, n) for L in lengths]
        for L in (1, o, o + 1, 3 * o + 2):   # what the restated convolution yields before it is cut is never shorter
            assert len(R.resample(torch.zeros(L), *rates)) == R.target_length(L, *rates) == rs.target_length(L)


def test_keywords_are_torchaudios_and_bad_ones_raise():
    from artspeech_amd.phoneme_recognition import features as F
    assert list(inspect.signature(F.Resample.__init__).parameters)[1:] == ["orig_freq", "new_freq", "resampling_method",
                                                                           "lowpass_filter_width", "rolloff", "beta"]
    d = {k: p.default for k, p in inspect.signature(F.Resample.__init__).parameters.items() if k != "self"}
    assert d == dict(orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, beta=None)
    assert list(inspect.signature(F.resample).parameters)[:3] == ["waveform", "orig_freq", "new_freq"]
    assert F.KAISER_BETA == 14.769656459379492
    for bad in (dict(resampling_method="linear"), dict(lowpass_filter_width=0), dict(rolloff=0.0), dict(orig_freq=44100.5)):
        with pytest.raises(ValueError, match="Resample"):
            F.Resample(**{"orig_freq": 44100, "new_freq": 16000, **bad})
    rs = F.Resample(44100, 16000)
    for call in (lambda: rs(torch.zeros(2, 400)), lambda: rs.resample_batch(torch.zeros(2, 400), [400, 300]),
                 lambda: F.resample(torch.zeros(400), 44100, 16000), lambda: F.Resample(16000, 16000)(torch.zeros(4))):
        with pytest.raises(RuntimeError, match="MI355X"):   # there is no host path
            call()
    assert F.resampler(44100, 16000) is F.resampler(44100, 16000) and F.resampler(44100, 16000, rolloff=0.9) is not F.resampler(44100, 16000)
    with open(os.path.join(ROOT, "include", "artspeech_hip.h")) as f:
        header = f.read()
    for name, value in (("PHASES", F.MAX_PHASES), ("BAND", F.MAX_BAND), ("ROW", F.MAX_ROW)):
        assert int(re.search(rf"#define AS_RESAMPLE_MAX_{name} (\w+)", header).group(1), 0) == value


def test_limits_are_refused_before_any_launch():
    """as_resample_fwd without a device: the addresses are never read, because every refusal comes before the launch"""
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition.features import MAX_BAND, MAX_PHASES, MAX_ROW
    ok = dict(x=16, x_int16=0, x_pitch=100, n_samples=16, B=1, o=3, n=2, coef=16, first=16, band=19, width=10, lead_min=-9, lead_max=-8,
              pad=0.0, out=16, out_pitch=100, m_max=100, lengths_out=None)
    for change, message in ((dict(n=MAX_PHASES + 1), "phases"), (dict(band=MAX_BAND + 1), "band"), (dict(x_pitch=MAX_ROW + 1), "row limit"),
                            (dict(out_pitch=MAX_ROW + 1, m_max=MAX_ROW + 1), "row limit"), (dict(o=MAX_ROW + 1), "row limit"),
                            (dict(o=60000, n=1, band=MAX_BAND, lead_min=-20000, lead_max=0), "leads"),
                            (dict(o=60000, n=1, band=MAX_BAND, lead_min=-12000, lead_max=0), "stages"), (dict(B=65536), "grid")):
        with pytest.raises(RuntimeError, match=rf"^as_resample_fwd failed \(code -2\): .*{message}"):
            _lib.call("as_resample_fwd", *{**ok, **change}.values(), stream=0)
    for change in (dict(x=None), dict(out_pitch=99), dict(band=0), dict(lead_max=-10)):
        with pytest.raises(RuntimeError, match=r"^as_resample_fwd failed \(code -1\): .*bad argument"):
            _lib.call("as_resample_fwd", *{**ok, **change}.values(), stream=0)
    assert _lib.call("as_resample_tile", 441, 160, 34, 1) == 1024 and _lib.call("as_resample_span", 1024, 441, 160, 34, 1) == 2856
    assert _lib.call("as_resample_tile", 24, 1, 293, 0) == 256 and _lib.call("as_resample_tile", 3, MAX_PHASES + 1, 8, 1) == 0


def test_planner_under_the_sanitizers(tmp_path):
    """the limit and tile chooser is C++ (csrc/resample_plan.cpp): a stand-alone program with its own main, built with the address
    and undefined-behaviour sanitizers and run on the CPU; the table builder is Python (features.py)"""
    exe = str(tmp_path / "resample_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan",   # the runtime inside the program: whatever else a machine loads into its processes
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "artspeech_amd", "csrc", "resample_plan.cpp"),
                           os.path.join(ROOT, "tests", "resample_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    m = re.fullmatch(r"sweep: 20000 plans, (\d+) refused, (\d+) outputs inside their spans\n", run.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 100000, run.stdout


def test_read_wav_round_trip(tmp_path):
    from artspeech_amd.phoneme_recognition.datasets import read_wav
    rng = np.random.default_rng(0)
    mono = rng.integers(-32768, 32768, (1000, 1)).astype(np.int16)
    mono[:2, 0] = (-32768, 32767)
    _write_wav(tmp_path / "mono.wav", mono, 44100)
    samples, rate = read_wav(tmp_path / "mono.wav")
    assert rate == 44100 and samples.dtype == torch.int16 and samples.shape == (1000,) and np.array_equal(samples.numpy(), mono[:, 0])
    stereo = rng.integers(-32768, 32768, (777, 2)).astype(np.int16)
    _write_wav(tmp_path / "stereo.wav", stereo, 22050)
    samples, rate = read_wav(str(tmp_path / "stereo.wav"))
    assert rate == 22050 and samples.shape == (777,) and np.array_equal(samples.numpy(), stereo[:, 0]), "the first channel"
    _write_wav(tmp_path / "deep.wav", rng.integers(-2 ** 23, 2 ** 23, (50, 1)), 48000, width=3)
    with pytest.raises(ValueError, match="24-bit"):
        read_wav(tmp_path / "deep.wav")


def _recordings(tmp_path, rates=(44100, 16000, 22050)):
    """a manifest of one WAV file per rate, 0.5 s of a 440 Hz tone each, with three intervals"""
    entries = []
    for idx, rate in enumerate(rates):
        n = rate // 2 + idx
        tone = np.round(8000 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)).astype(np.int16)
        _write_wav(tmp_path / f"utt{idx}.wav", np.stack([tone, -tone], axis=1) if idx == 0 else tone[:, None], rate)
        entries.append({"audio_filepath": f"utt{idx}.wav", "phonemes": [["ph00", 0.0, 0.2], ["zz", 0.2, 0.3], ["ph03", 0.3, 0.5]]})
    manifest = tmp_path / "manifest.json"
    manifest.write_text(json.dumps(entries))
    return manifest, entries


def test_manifest_items_carry_the_synthetic_keys_and_the_rate(tmp_path):
    from artspeech_amd.phoneme_recognition.datasets import RecordedAcousticRecognitionDataset, SyntheticAcousticRecognitionDataset
    vocab = _vocab()
    manifest, entries = _recordings(tmp_path)
    ds = RecordedAcousticRecognitionDataset(str(manifest), vocab, voiced_tokens=["ph00"])
    assert len(ds) == 3 and len(RecordedAcousticRecognitionDataset([dict(e, audio_filepath=str(tmp_path / e["audio_filepath"])) for e in entries],
                                                                   vocab)) == 3
    synthetic_keys = set(SyntheticAcousticRecognitionDataset(1, vocab, min_seconds=0.1, max_seconds=0.2)[0])
    for idx, rate in enumerate((44100, 16000, 22050)):
        item = ds[idx]
        assert set(item) == synthetic_keys | {"sample_rate"}
        n = rate // 2 + idx
        assert item["sample_rate"] == rate and item["waveform_length"] == n and item["audio_duration"] == n / rate
        assert item["waveform"].dtype == torch.int16 and item["waveform"].shape == (n,) and 7900 < int(item["waveform"].abs().max()) <= 8000
        assert item["phonemes_with_time"] == [("ph00", 0.0, 0.2), ("zz", 0.2, 0.3), ("ph03", 0.3, 0.5)]
        assert item["phoneme_tokens"] == [vocab["ph00"], vocab["<unk>"], vocab["ph03"]]
        assert item["ctc_target"].tolist() == item["phoneme_tokens"] and item["ctc_target_length"] == 3
        T = item["articulatory_target_length"]
        assert T == int(item["audio_duration"] * 50) == len(item["articulatory_target"]) == len(item["voicing"])
        want = [vocab["ph00"] if (f + 0.5) / 50 < 0.2 else vocab["<unk>"] if (f + 0.5) / 50 < 0.3 else vocab["ph03"] for f in range(T)]
        assert item["articulatory_target"].tolist() == want and item["articulatory_target"].dtype == torch.int64
        assert torch.equal(item["voicing"], (item["articulatory_target"] == vocab["ph00"]).float())
    with pytest.raises(ValueError, match="audio_filepath"):
        RecordedAcousticRecognitionDataset([{"phonemes": []}], vocab)


def test_synthetic_waveforms_at_a_foreign_rate():
    from artspeech_amd.phoneme_recognition.datasets import SyntheticAcousticRecognitionDataset
    vocab = _vocab()
    kw = dict(min_seconds=0.3, max_seconds=0.6, seed=5)
    plain, foreign = SyntheticAcousticRecognitionDataset(3, vocab, **kw), SyntheticAcousticRecognitionDataset(3, vocab, orig_sample_rate=44100, **kw)
    up = SyntheticAcousticRecognitionDataset(3, vocab, orig_sample_rate=8000, **kw)
    assert plain.orig_sample_rate is None and plain.sample_rate == 16000 and "sample_rate" not in plain[0]
    assert foreign.sample_rate == foreign.orig_sample_rate == 44100 and up.sample_rate == 8000
    # below 0.45 of the LOWER rate, whichever side it is on: the prototypes survive the low-pass
    assert torch.equal(foreign.frequencies, plain.frequencies) and float(foreign.frequencies.max()) <= 0.45 * 16000
    assert float(up.frequencies.max()) <= 0.45 * 8000 < float(plain.frequencies.max())
    for i in range(3):
        item = foreign[i]
        assert set(item) == set(plain[i]) | {"sample_rate"} and item["sample_rate"] == 44100
        n = item["waveform_length"]
        assert int(0.3 * 44100) <= n <= int(0.6 * 44100) + 1 and item["waveform"].shape == (n,) and item["audio_duration"] == n / 44100
        spans = item["phonemes_with_time"]
        assert spans[0][1] == 0.0 and spans[-1][2] == item["audio_duration"]                        # labels stay in seconds
        assert all(0.06 - 1e-4 <= e - s <= 0.2 + 1e-4 for _, s, e in spans[:-1])
        assert item["articulatory_target_length"] == int(item["audio_duration"] * 50)
    with pytest.raises(ValueError, match="orig_sample_rate"):
        SyntheticAcousticRecognitionDataset(1, vocab, orig_sample_rate=0)


def test_new_configs_are_main_arguments_and_differ_in_the_rate_alone():
    import align_phoneme_recognition as A
    import test_phoneme_recognition as TE
    import train_phoneme_recognition as T
    for script, kind in ((T, "train"), (TE, "test"), (A, "align")):
        with open(os.path.join(ROOT, "configs", f"{kind}_recognizer_acoustic_44k_synthetic.yaml")) as f:
            cfg = yaml.safe_load(f)
        with open(os.path.join(ROOT, "configs", f"{kind}_recognizer_acoustic_synthetic.yaml")) as f:
            base = yaml.safe_load(f)
        assert set(cfg) <= set(inspect.signature(script.main).parameters)
        assert cfg["synthetic"].pop("orig_sample_rate") == 44100 and cfg["num_workers"] == 0 and cfg["datadir"] == "synthetic"
        mel = cfg["melspec"] if kind == "train" else cfg["synthetic"]["melspec"]
        assert mel["sample_rate"] == 16000
        differ = {k for k in cfg if cfg[k] != base[k]}
        assert differ == ({"results_dir"} if kind == "train" else {"state_dict_filepath", "save_dir"}), differ
        if kind != "train":
            assert cfg["state_dict_filepath"] == "results/recognizer_acoustic_44k_synthetic/best_model.pt"


def test_make_dataset_takes_the_foreign_rate_and_the_manifest(tmp_path, monkeypatch):
    import train_phoneme_recognition as T
    from artspeech_amd.phoneme_recognition.datasets import (RecordedAcousticRecognitionDataset, SyntheticAcousticRecognitionDataset,
                                                            acoustic_collate_fn, collate_fn)
    vocab = _vocab()
    small = {"n_fft": 256, "win_length": 256, "hop_length": 64, "n_mels": 20}
    ds = T._make_dataset("synthetic", "artspeech2", {"num_sentences": 3}, vocab, T.Feature.MELSPEC, None,
                         {"min_seconds": 0.3, "max_seconds": 0.6, "orig_sample_rate": 44100, "melspec": small}, 7)
    assert isinstance(ds, SyntheticAcousticRecognitionDataset) and ds.sample_rate == 44100 and ds.melspectrogram.sample_rate == 16000
    assert ds[0]["sample_rate"] == 44100 and ds[0]["melspectrogram"] is ds.melspectrogram
    manifest, _ = _recordings(tmp_path)
    rec = T._make_dataset("recordings", "artspeech2", {"manifest": str(manifest)}, vocab, T.Feature.MELSPEC, None, {"framerate": 25, "melspec": small}, 0)
    assert isinstance(rec, RecordedAcousticRecognitionDataset) and len(rec) == 3 and rec.framerate == 25
    assert (rec.melspectrogram.n_fft, rec.melspectrogram.n_mels, rec.melspectrogram.sample_rate) == (256, 20, 16000)
    assert rec[0]["melspectrogram"] is rec.melspectrogram and rec[0]["sample_rate"] == 44100
    with pytest.raises(ValueError, match="manifest"):
        T._make_dataset("recordings", "artspeech2", {"num_sentences": 3}, vocab, T.Feature.MELSPEC, None, None, 0)
    with pytest.raises(ValueError, match="manifest"):
        T._make_dataset("recordings", "artspeech2", {"manifest": str(manifest)}, vocab, T.Feature.VOCAL_TRACT, None, None, 0)
    with pytest.raises(ValueError, match="voicing"):
        T._make_dataset("recordings", "artspeech2", {"manifest": str(manifest)}, vocab, T.Feature.MELSPEC, ["ph00"], None, 0)
    # the collate function of either data set launches on the device: no host path, no worker process
    with pytest.raises(ValueError, match="num_workers"):
        T.make_collate_fn("recordings", T.Feature.MELSPEC, 2, rec)
    for items in ([ds[0], ds[1]], [rec[0], rec[1], rec[2]]):
        with pytest.raises(RuntimeError, match="MI355X"):
            collate_fn(items, [T.Feature.MELSPEC])
    import torch.utils.data
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    for items in ([ds[0], ds[1]], [rec[0], rec[1]]):
        with pytest.raises(ValueError, match="num_workers"):
            collate_fn(items, [T.Feature.MELSPEC])
        with pytest.raises(ValueError, match="num_workers"):
            acoustic_collate_fn(items, ds.melspectrogram)


def test_header_declares_and_binding_binds_the_entry_point():
    from artspeech_amd import _lib, build
    with open(os.path.join(ROOT, "include", "artspeech_hip.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint as_resample_fwd\s*\(", header) and re.search(r"\bint32_t as_resample_tile\s*\(", header)
    assert "datasets.py:124-126" in text, "the reference call site is not cited"
    L = _lib.lib()
    for name in ("as_resample_fwd", "as_resample_tile", "as_resample_span"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    res, args = _lib.PROTOTYPES["as_resample_fwd"]
    assert len(args) == 19 and args[-1] is _lib.Stream
    for name in ("resample.hip", "resample_plan.cpp"):
        assert build.SOURCES[name] == [] and os.path.exists(os.path.join(build.CSRC, name))
