"""Host-side pieces of the speech synthesis from the tube (no GPU): the restatement of tests/vt_synth_fp64.py against the closed
forms its definition has and the properties it promises, the glue's restatement on hand-made inputs, the WAV writer, the bindings
and the scripts' configs."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import vt_acoustics_fp64 as A
import vt_synth_fp64 as R
from conftest import ROOT

FS = 44100.0


def impulse_response(areas, n, **kw):
    """The static ladder's response to a unit impulse at sample 0, without differencing."""
    areas = np.asarray(areas, np.float64)
    src = np.zeros((1, n))
    src[0, 0] = 1.0
    out, status = R.ladder(areas[None, None, :], [len(areas)], [1], n, src, radiation=0, **kw)
    assert status.tolist() == [0]
    return out[0]


def first_peaks(x, nfft, count, above):
    """Frequencies (Hz at FS) of the first ``count`` local maxima of |FFT| that exceed ``above`` x the largest value."""
    spectrum = np.abs(np.fft.rfft(x, nfft))
    peaks = [i for i in range(1, len(spectrum) - 1) if spectrum[i] > spectrum[i - 1] and spectrum[i] >= spectrum[i + 1]
             and spectrum[i] > above * spectrum.max()]
    return np.array(peaks[:count]) * FS / nfft


# ---------------------------------------------------------------------------------------------------- the ladder
def test_uniform_tube_resonates_at_odd_quarters_of_its_delay():
    """K = 22 equal sections, r_g = 0.97, r_l = -0.97, mu = 1: the first four peaks lie at (2n - 1) fs / 4K within one bin of a
    2^17-point FFT of 8192 samples: 500.98 / 1503.29 / 2505.59 / 3507.89 Hz against 501.14 / 1503.41 / 2505.68 / 3507.95 Hz."""
    K, nfft = 22, 1 << 17
    got = first_peaks(impulse_response(np.ones(K), 8192, r_g=0.97, r_l=-0.97, mu=1.0), nfft, 4, 0.3)
    want = (2 * np.arange(1, 5) - 1) * FS / (4 * K)
    print("uniform ladder:", got, "closed form", want)
    assert np.abs(got - want).max() <= FS / nfft


def test_static_random_tube_against_the_direct_solve():
    """Random areas, K = 9, partial reflections: the DFT of the impulse response equals the direct solve of the 2K steady-state
    equations at z = exp(j omega) to 1e-12 relative (measured 1.9e-14; the response has decayed to 1e-39 at 4096 samples)."""
    areas = np.exp(np.random.default_rng(1).standard_normal(9))
    n = 4096
    h = impulse_response(areas, n, r_g=0.6, r_l=-0.7, mu=0.99)
    assert np.abs(h[-100:]).max() < 1e-30
    direct = R.steady_state(areas, 2 * np.pi * np.arange(n) / n, 0.6, -0.7, 0.99)
    error = np.abs(np.fft.fft(h) - direct).max() / np.abs(direct).max()
    print(f"direct solve: {error:.2e}")
    assert error <= 1e-12


@pytest.mark.parametrize("K,seed", [(12, 0), (20, 1), (22, 2)])
def test_peaks_against_the_frequency_domain_formants(K, seed):
    """A static, lightly damped ladder (r_g = 1, r_l = -0.99, mu = 0.999, 16384 samples: the tail is below 1e-7) against
    vt_acoustics_fp64.formants of the same tube, K sections of c / fs with the ideal open end.  mu scales every pole's radius
    and moves no pole's frequency; the peak of |H| still leans towards its neighbours' skirts by about bandwidth^2 / spacing,
    (35 Hz / 2)^2 / 1 kHz ~ 0.3 Hz.  Measured over 18 tubes (K = 12, 20, 22, six draws each) with a 2^17-point FFT (bin 0.336 Hz):
    at most 0.44 Hz = 1.31 bins (with mu = 0.998, r_l = -0.98: 1.6 Hz; the shift follows the damping).  Tolerance: two bins
    plus the formants' last bracket."""
    nfft = 1 << 17
    areas = np.exp(np.random.default_rng(seed).uniform(np.log(0.3), np.log(8.0), K))
    h = impulse_response(areas, 16384, r_g=1.0, r_l=-0.99, mu=0.999)
    assert np.abs(h[-50:]).max() <= 1e-6 * np.abs(h).max()
    got = first_peaks(h, nfft, 4, 0.01)
    freq, _, found, status = A.formants(areas[None, :], np.full((1, K), A.C_SOUND / FS), None, f0=10.0, df=10.0, F=2000, radiation=0,
                                        n_formants=4, rounds=3)
    assert found.tolist() == [4] and status.tolist() == [0]
    shift = np.abs(got - freq[0]).max()
    print(f"K = {K}: peaks {got}, formants {freq[0]}, shift {shift:.3f} Hz = {shift / (FS / nfft):.2f} bins")
    assert shift <= 2 * FS / nfft + A.bracket_width(10.0, 3)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_time_varying_ladder_is_passive(seed):
    """Areas exp(N(0, 1)) per frame, r_g = 0.9, r_l = -0.9, mu = 1, a burst of ten samples: the last 300 of 3000 samples stay
    below 1e-3 of the first 300 (measured over the three draws: 2e-8) -- interpolating k, a convex combination, never adds energy."""
    T, S, K = 30, 100, 12
    areas = np.exp(np.random.default_rng(seed).standard_normal((1, T, K)))
    src = np.zeros((1, T * S))
    src[0, :10] = 1.0
    out, _ = R.ladder(areas, [K], [T], S, src, r_g=0.9, r_l=-0.9, mu=1.0, radiation=0)
    ratio = np.abs(out[0, -300:]).max() / np.abs(out[0, :300]).max()
    print(f"passivity, draw {seed}: {ratio:.2e}")
    assert ratio <= 1e-3


def test_ladder_conventions():
    """Differencing, the held last frame, zero beyond n_b, ragged sections in one batch equal to each alone, status bits."""
    rng = np.random.default_rng(3)
    areas = np.exp(0.5 * rng.standard_normal((2, 3, 7)))
    src = rng.standard_normal((2, 3 * 8 + 2))
    plain, _ = R.ladder(areas, [7, 4], [3, 2], 8, src, radiation=0)
    diff, status = R.ladder(areas, [7, 4], [3, 2], 8, src, radiation=1)
    assert status.tolist() == [0, 0] and (plain[0, 24:] == 0).all() and (plain[1, 16:] == 0).all()
    assert np.array_equal(diff[0, 1:24], plain[0, 1:24] - plain[0, :23]) and diff[0, 0] == plain[0, 0]
    alone, _ = R.ladder(areas[1:, :, :4], [4], [2], 8, src[1:], radiation=0)
    assert np.array_equal(alone[0], plain[1])
    held = areas.copy()
    held[0, 2] = 99.0   # frame t' of the last frame is the last frame itself; frame 2 is only ever approached
    same, _ = R.ladder(held, [7, 4], [2, 2], 8, src, radiation=0)
    short, _ = R.ladder(areas, [7, 4], [2, 2], 8, src, radiation=0)
    assert np.array_equal(same, short)
    areas[0, 1, 2], areas[1, 0, 1] = 1e-6, np.nan
    out, status = R.ladder(areas, [7, 4], [3, 2], 8, src)
    assert status.tolist() == [1, 2] and np.isnan(out[1, :16]).all() and (out[1, 16:] == 0).all() and np.isfinite(out[0]).all()


# ---------------------------------------------------------------------------------------------------- the source
def test_pulse_is_continuous_at_its_three_breakpoints():
    eps = 2.0 ** -40
    for at in (0.0, R.RISE, R.RISE + R.FALL):
        below, above = R.pulse(np.array([(at - eps) % 1.0])), R.pulse(np.array([at + eps]))
        assert abs(float(below[0]) - float(above[0])) <= 1e-10, at
    assert float(R.pulse(np.array([R.RISE]))[0]) == 1.0 and float(R.pulse(np.array([0.0]))[0]) == 0.0
    assert float(R.pulse(np.array([0.9]))[0]) == 0.0 and abs(float(R.pulse(np.array([R.RISE + R.FALL - eps]))[0])) < 1e-10


def test_phase_closed_form_equals_the_running_sum():
    rng = np.random.default_rng(4)
    T, S, fs = 40, 37, 1850.0
    f0 = rng.uniform(-30.0, 300.0, T)   # frames below 0 are read as 0
    for F in (40, 7, 1):
        closed = R.phase(f0, F, S, fs)
        summed = R.phase_running_sum(f0, F, S, fs)
        error = np.abs(closed - summed).max()
        print(f"phase, {F} frames: {float(summed[-1]):.2f} cycles, closed form off by {float(error):.2e}")
        assert error <= 2.0 ** -52 * 8 * (1 + float(summed[-1]))
    assert (np.diff(R.phase(f0, 40, S, fs)) >= 0).all()


def test_noise_range_streams_and_seed():
    n = np.arange(100000)
    a = R.noise(5, 0, 0, n)
    assert a.dtype == np.float64 and a.min() >= -1.0 and a.max() < 1.0 and abs(a.mean()) < 0.01 and abs(a.std() - 3 ** -0.5) < 0.01
    assert np.array_equal(a, R.noise(5, 0, 0, n))
    for other in (R.noise(5, 1, 0, n), R.noise(5, 0, 1, n), R.noise(6, 0, 0, n)):
        assert not np.array_equal(a, other) and abs(np.corrcoef(a, other)[0, 1]) < 0.02
    # the splitmix64 finaliser, by hand for one index: idx = ((2 b + stream) << 40) | n
    z = (5 + ((((2 * 3 + 1) << 40) | 17) + 1) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    assert float(R.noise(5, 1, 3, [17])[0]) == 2.0 * ((z >> 11) * 2.0 ** -53) - 1.0


def test_source_shape_and_status():
    f0, va, asp = np.full((2, 4), 100.0), np.ones((2, 4)), np.zeros((2, 4))
    out, status, cycles = R.source(f0, va, asp, [4, 2], 50, 1000.0, pitch=203)
    assert out.shape == (2, 203) and status.tolist() == [0, 0] and (out[0, 200:] == 0).all() and (out[1, 100:] == 0).all()
    assert abs(cycles[0] - 19.9) < 1e-9 and out.min() >= 0.0 and abs(out.max() - 1.0) < 1e-12
    assert np.allclose(out[0, :10], out[0, 10:20], atol=1e-12)   # 100 Hz at 1 kHz: a period of ten samples
    va[1, 1] = np.nan
    out, status, _ = R.source(f0, va, asp, [4, 2], 50, 1000.0)
    assert status.tolist() == [0, 2] and np.isnan(out[1, :100]).all() and (out[1, 100:] == 0).all()


# ---------------------------------------------------------------------------------------------------- the glue
def test_equal_sections_by_hand():
    """Two sections of 6 and 10 cm (areas 1 and 4) at fs / c = 1 / 4 per cm: K = 4 slices of 4 cm with midpoints 2, 6, 10, 14 --
    the end of a section belongs to the next one."""
    areas = np.array([[[1.0, 4.0, 9.0], [2.0, 5.0, 9.0], [np.nan, 1.0, 1.0], [3.0, 3.0, 9.0]]])
    lengths = np.array([[[6.0, 10.0, 1.0], [8.0, 8.0, 1.0], [8.0, 8.0, 1.0], [4.0, 12.0, 1.0]]])
    counts = np.array([[2, 2, 2, 2]])
    eq, sections, tract, replaced = R.equal_sections(areas, lengths, counts, [4], 8750.0, c=35000.0)
    assert sections.tolist() == [4] and replaced.tolist() == [1] and tract.tolist() == [[16.0, 16.0, 16.0]]
    assert eq[0].tolist() == [[1, 4, 4, 4], [2, 2, 5, 5], [2, 2, 5, 5], [3, 3, 3, 3]]
    eq, sections, _, replaced = R.equal_sections(areas[:, 2:], lengths[:, 2:], counts[:, 2:], [2], 8750.0, c=35000.0)
    assert eq[0].tolist() == [[3, 3, 3, 3], [3, 3, 3, 3]] and replaced.tolist() == [1]    # at the start: the nearest later one
    eq, sections, tract, _ = R.equal_sections(areas, lengths, counts, [4], 100.0, c=35000.0)
    assert sections.tolist() == [2] and eq[0, 0].tolist() == [1, 4]                       # clamped to two sections
    eq, sections, tract, replaced = R.equal_sections(areas[:, 2:3], lengths[:, 2:3], counts[:, 2:3], [1], 8750.0)
    assert np.isnan(eq).all() and np.isnan(tract).all() and sections.tolist() == [2] and replaced.tolist() == [1]


def test_frication_control_by_hand():
    areas = np.array([[[0.05, 1.0, 0.1, 0.1, 2.0, 0.01], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [1.0, 1e-6, 1.0, 1.0, 1.0, 1.0],
                       [1.0, 1.0, 1.0, 1.0, 0.15, 1.0]]])
    where, q = R.frication_control(areas, [6], 0.4, critical_area=0.2)
    # the glottis' and the lips' own sections are not looked at; the lowest index among equals; a closure is silent
    assert where.tolist() == [[3, -1, -1, 5]] and np.allclose(q, [[0.2, 0.0, 0.0, 0.1]], rtol=1e-12)
    where, q = R.frication_control(areas[:, :, :2], [2], 0.4)
    assert (where == -1).all() and (q == 0).all()


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from artspeech_amd import vocal_tract_synthesis as V
    x = torch.ones(1, 2, 3, dtype=torch.float64)
    for call in (lambda: V.equal_sections(x, x, torch.ones(1, 2), [2], 16000.0), lambda: V.frication_control(x, [3], 0.1),
                 lambda: V.glottal_source(torch.ones(1, 2), 1.0, 0.0, [2], 10, 500.0),
                 lambda: V.waveguide(x, [3], [2], 10, torch.zeros(1, 20, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="radiation"):
        V.waveguide(x, [3], [2], 10, torch.zeros(1, 20, dtype=torch.float64), radiation="piston")
    p = inspect.signature(V.waveguide).parameters
    assert (p["r_g"].default, p["r_l"].default, p["mu"].default, p["min_area"].default) == (R.R_GLOTTIS, R.R_LIPS, R.MU, R.MIN_AREA)
    p = inspect.signature(V.glottal_source).parameters
    assert (p["rise"].default, p["fall"].default) == (R.RISE, R.FALL) == (0.40, 0.16)
    p = inspect.signature(V.synthesize_speech).parameters
    assert (p["f0_start"].default, p["f0_end"].default, p["critical_area"].default) == (120.0, 90.0, 0.2)
    assert V.MAX_SECTIONS == 64 and V.SOUND_SPEED == R.SOUND_SPEED


def test_write_wav_round_trips_through_read_wav(tmp_path):
    from artspeech_amd.phoneme_recognition.datasets import read_wav, write_wav
    x = torch.tensor([0, 1, -1, 32767, -32768, 1234, -4321], dtype=torch.int16)
    back, rate = read_wav(write_wav(tmp_path / "a.wav", x, 44100))
    assert rate == 44100 and back.dtype == torch.int16 and torch.equal(back, x)
    y = torch.tensor([0.0, 0.5, -0.5, 0.99999, 1.5, -1.0, -2.0, 1.5 / 32768, 2.5 / 32768], dtype=torch.float32)
    back, rate = read_wav(write_wav(tmp_path / "b.wav", y, 16000))
    assert rate == 16000 and back.tolist() == [0, 16384, -16384, 32767, 32767, -32768, -32768, 2, 2]   # clipped; halves to even
    assert torch.equal(read_wav(write_wav(tmp_path / "c.wav", back.float() / 32768.0, 8000))[0], back)
    with pytest.raises(ValueError, match="non-finite"):
        write_wav(tmp_path / "d.wav", torch.tensor([0.0, float("nan")]), 8000)
    with pytest.raises(ValueError, match="sample rate"):
        write_wav(tmp_path / "d.wav", x, 22050.5)


# ---------------------------------------------------------------------------------------------------- bindings, configs
def test_bindings_carry_the_header_types():
    from artspeech_amd import _lib
    P, S, I32, I64, D, U64 = ctypes.c_void_p, _lib.Stream, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_uint64
    assert _lib.PROTOTYPES["as_vt_glottal_source"] == (I32, [P, P, P, P, I32, I32, I32, D, U64, D, D, P, I64, P, S])
    assert _lib.PROTOTYPES["as_vt_waveguide"] == (I32, [P, I64, I64, I64, P, P, I32, I32, I32, I32, P, P, P, U64, D, D, D, D, I32, P, P,
                                                        I64, P, S])
    _lib.lib()
    assert _lib._bound["as_vt_waveguide"][1:] == (True, True) and _lib._bound["as_vt_glottal_source"][1:] == (True, True)
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    source = open(os.path.join(ROOT, "artspeech_amd", "csrc", "vt_synth.hip")).read()
    assert "ASSUMPTION" in header[header.index("Speech from the tube"):header.index("int as_vt_glottal_source")]
    assert "ASSUMPTION" in source and "include/artspeech_hip.h" in source


def test_library_refuses_bad_arguments_before_any_launch():
    """What needs no device: the checks that come before the section counts are read back."""
    from artspeech_amd import _lib
    ok = dict(areas=8, strides=(6, 3, 1), sections=8, frames=8, B=1, T=2, Kmax=3, S=4, source=8, where=None, gain=None, seed=0,
              r=(0.75, -0.85, 0.999, 1e-4), radiation=1, out64=None, out32=None, pitch=8, status=None)

    def waveguide(**change):
        a = {**ok, **change}
        return _lib.call("as_vt_waveguide", a["areas"], *a["strides"], a["sections"], a["frames"], a["B"], a["T"], a["Kmax"], a["S"],
                         a["source"], a["where"], a["gain"], a["seed"], *a["r"], a["radiation"], a["out64"], a["out32"], a["pitch"],
                         a["status"], stream=0)
    for change, text in ((dict(S=0), "S = 0"), (dict(pitch=7), "pitch"), (dict(radiation=2), "radiation"), (dict(where=8), "come together"),
                         (dict(r=(0.75, -0.85, 0.999, 0.0)), "min_area"), (dict(Kmax=0), "Kmax"), (dict(sections=None), "NULL")):
        with pytest.raises(RuntimeError, match=text):
            waveguide(**change)
    assert waveguide(B=0) == 0   # an empty batch launches nothing

    def source(**change):
        a = {**dict(B=1, T=2, S=4, fs=200.0, rise=0.4, fall=0.16, pitch=8, f0=8), **change}
        return _lib.call("as_vt_glottal_source", a["f0"], 8, 8, 8, a["B"], a["T"], a["S"], a["fs"], 0, a["rise"], a["fall"], 8, a["pitch"],
                         None, stream=0)
    for change, text in ((dict(S=0), "S = 0"), (dict(pitch=7), "pitch"), (dict(fs=0.0), "sample_rate"), (dict(rise=0.9), "rise"),
                         (dict(f0=None), "NULL")):
        with pytest.raises(RuntimeError, match=text):
            source(**change)
    assert source(B=0) == 0


def test_script_configs():
    import yaml

    import vocal_tract_speech as S
    from artspeech_amd.area_function import build_semipolar_grid
    assert not S.__name__.startswith(("train_", "test_"))
    with open(os.path.join(ROOT, "configs", "vocal_tract_speech_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= set(inspect.signature(S.main).parameters)
    assert set(cfg["grid"]) <= set(inspect.signature(build_semipolar_grid).parameters)
    with open(os.path.join(ROOT, "configs", "vocal_tract_formants_synthetic.yaml")) as f:
        formants = yaml.safe_load(f)
    assert all(cfg[k] == formants[k] for k in ("datadir", "database_name", "grid", "alpha", "beta"))
    from artspeech_amd.settings import DATASET_CONFIG
    from artspeech_amd.training import build_vocabulary
    assert round(cfg["sample_rate"] / DATASET_CONFIG[cfg["database_name"]].FRAMERATE) == 882
    assert set(cfg["voiced_tokens"]) < set(build_vocabulary(None))
    with open(os.path.join(ROOT, "configs", "train_recognizer_synthesised_speech_synthetic.yaml")) as f:
        train = yaml.safe_load(f)
    import train_phoneme_recognition as trainer
    assert set(train) <= set(inspect.signature(trainer.main).parameters)
    assert train["datadir"] == "recordings" and train["feature"] == "melspec"
    manifest = os.path.join(cfg["datadir"], "manifest.json")
    assert all(train[k] == {"manifest": manifest} for k in ("train_seq_dict", "valid_seq_dict", "test_seq_dict"))
    assert train["melspec"]["sample_rate"] == cfg["model_sample_rate"]
    assert S.phoneme_intervals(["a", "a", "b", "a"], 50) == [["a", 0.0, 0.04], ["b", 0.04, 0.06], ["a", 0.06, 0.08]]
