"""as_vt_glottal_source and as_vt_waveguide on the device against the numpy restatement (tests/vt_synth_fp64.py).

The ladder.  Per utterance the yardstick is measured, not fixed: e64 = max |restatement in float64 - restatement in longdouble| /
max |longdouble out|.  The device's out64 must stay within 16 max(e64, K 2^-52) of the longdouble restatement by the same norm:
its fused multiply-adds are another rounding path of the same length, not a less accurate one -- hence a constant factor, not a
new scale.  Where the restatement is identically 0 the device is exactly 0, and out32 is out64 rounded to float32, bit for bit.

The source, by the same scheme, with the floor 2^-52 (1 + cycles) pi / (2 fall): one ulp of the total phase times the pulse's
steepest slope (the amplitudes of the cases are at most 1).  The noise term is exact."""
import json
import os

import numpy as np
import pytest
import torch

import vt_synth_fp64 as R

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 67   # elements behind the last row: nothing behind the pitch is written


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def on(dev, x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def launch_ladder(dev, areas, sections, frames, S, source, where=None, gain=None, seed=0, r_g=R.R_GLOTTIS, r_l=R.R_LIPS, mu=R.MU,
                  min_area=R.MIN_AREA, radiation=1, outputs=("out64", "out32"), expect=0):
    """The C ABI as it is.  The outputs are filled with a sentinel first and end in a guard, so that an element the kernel left
    alone shows.  Returns {name: (B, pitch) numpy array}, the status and the guards; ``expect`` is the return code."""
    from artspeech_amd import _lib
    B, T, Kmax = areas.shape
    pitch = source.shape[1]
    a = on(dev, areas, np.float64)
    bufs = {"out64": torch.full((B * pitch + GUARD,), SENTINEL, dtype=torch.float64, device=dev) if "out64" in outputs else None,
            "out32": torch.full((B * pitch + GUARD,), SENTINEL, dtype=torch.float32, device=dev) if "out32" in outputs else None}
    status = torch.full((B,), -5, dtype=torch.int32, device=dev)
    args = ("as_vt_waveguide", a, T * Kmax, Kmax, 1, on(dev, sections, np.int32), on(dev, frames, np.int32), B, T, Kmax, S,
            on(dev, source, np.float64), on(dev, where, np.int32), on(dev, gain, np.float64), seed, float(r_g), float(r_l), float(mu),
            float(min_area), radiation, bufs["out64"], bufs["out32"], pitch, status)
    if expect == 0:
        _lib.call(*args)
    else:
        with pytest.raises(RuntimeError, match=rf"as_vt_waveguide failed \(code {expect}\)"):
            _lib.call(*args)
    torch.cuda.synchronize()
    out = {name: t.cpu().numpy() for name, t in bufs.items() if t is not None}
    for name, t in out.items():
        assert (t[B * pitch:] == SENTINEL).all(), f"{name}: written behind the last row"
    return {name: t[:B * pitch].reshape(B, pitch) for name, t in out.items()}, status.cpu().numpy()


def launch_source(dev, f0, voiced, asp, frames, S, fs, seed=0, rise=R.RISE, fall=R.FALL, pitch=None):
    from artspeech_amd import _lib
    B, T = f0.shape
    pitch = T * S if pitch is None else pitch
    buf = torch.full((B * pitch + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((B,), -5, dtype=torch.int32, device=dev)
    _lib.call("as_vt_glottal_source", on(dev, f0, np.float64), on(dev, voiced, np.float64), on(dev, asp, np.float64),
              on(dev, frames, np.int32), B, T, S, float(fs), seed, float(rise), float(fall), buf, pitch, status)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[B * pitch:] == SENTINEL).all(), "written behind the last row"
    return out[:B * pitch].reshape(B, pitch), status.cpu().numpy()


_REFERENCES = {}


def reference(index):
    """The restatement of one of R.CASES in float64 and in longdouble, computed once and shared by the tests that read it."""
    if index not in _REFERENCES:
        x = R.draw_case(R.CASES[index])
        kw = dict(inject_section=x["where"], inject_gain=x["gain"], seed=x["seed"], radiation=x["radiation"])
        o64, status = R.ladder(x["areas"], x["sections"], x["frames"], x["S"], x["source"], **kw)
        ol, _ = R.ladder(x["areas"], x["sections"], x["frames"], x["S"], x["source"], dtype=np.longdouble, **kw)
        _REFERENCES[index] = dict(x=x, o64=o64, ol=ol, status=status)
    return _REFERENCES[index]


def assert_parity(got, o64, ol, floor, what):
    """Per row: |got - ol| / max |ol| <= 16 max(e64, floor); a row whose restatement is identically 0 is exactly 0."""
    worst = 0.0
    for b in range(ol.shape[0]):
        scale = float(np.abs(ol[b]).max())
        if scale == 0.0:
            assert (got[b] == 0).all(), f"{what}: row {b} is identically 0 in the restatement"
            continue
        e64 = float(np.abs(o64[b] - ol[b]).max()) / scale
        tol = 16 * max(e64, float(floor[b]))
        err = float(np.abs(got[b].astype(np.longdouble) - ol[b]).max()) / scale
        print(f"{what}: row {b}: error / yardstick {err / tol:.3f} (error {err:.2e}, e64 {e64:.2e}, floor {float(floor[b]):.2e})")
        assert err <= tol, f"{what}: row {b}: {err:.3e} > {tol:.3e}"
        worst = max(worst, err / tol)
    return worst


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=R.CASE_IDS)
def test_ladder_against_the_restatement(dev, index):
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "longdouble is no wider than float64 on this machine"
    ref = reference(index)
    x = ref["x"]
    assert x["source"].shape[1] <= 5000
    got, status = launch_ladder(dev, x["areas"], x["sections"], x["frames"], x["S"], x["source"], x["where"], x["gain"], x["seed"],
                                radiation=x["radiation"])
    assert np.array_equal(status, ref["status"]) and (status == 0).all()
    assert_parity(got["out64"], ref["o64"], ref["ol"], x["sections"] * 2.0 ** -52, f"case {R.CASE_IDS[index]}")
    assert np.array_equal(got["out32"].view(np.uint32), got["out64"].astype(np.float32).view(np.uint32))
    n = np.asarray(x["frames"], np.int64) * x["S"]
    for b in range(len(n)):
        assert (got["out64"][b, n[b]:] == 0).all() and (got["out32"][b, n[b]:] == 0).all()


def test_the_cases_cover_what_they_are_meant_to():
    ks = {int(k) for c in R.CASES for k in c[3]}
    assert {1, 2, 16, 17, 32, 33, 63, 64} <= ks
    assert {1, 2, 63, 64, 65} <= {c[2] for c in R.CASES} and {1, 2, 9} <= {c[1] for c in R.CASES}
    assert max(c[0] for c in R.CASES) <= 5 and any(0 in c[4] for c in R.CASES) and {0, 1} == {c[5] for c in R.CASES}
    assert any(len(set(c[3])) > 1 for c in R.CASES) and any(len(set(c[4])) > 1 for c in R.CASES)
    x = R.draw_case(R.CASES[1])
    used = {(int(w), int(k)) for b, k in enumerate(x["sections"]) for w in x["where"][b, :x["frames"][b]]}
    assert any(w == 1 for w, _ in used) and any(w == k - 1 and k > 2 for w, k in used) and any(w == -1 for w, _ in used)


SOURCE_CASES = [(3, 9, 64, (9, 4, 0)), (2, 2, 1, (2, 1)), (2, 70, 65, (70, 65)), (1, 1, 63, (1,)), (2, 130, 2, (130, 129))]


@pytest.mark.parametrize("case", SOURCE_CASES, ids=lambda c: "B{}-T{}-S{}".format(*c[:3]))
def test_source_against_the_restatement(dev, case):
    B, T, S, frames = case
    rng = np.random.default_rng([B, T, S])
    fs = 50.0 * S if S >= 63 else 2000.0
    f0 = rng.uniform(-20.0, 0.2 * fs, (B, T))   # a few frames below 0: read as 0
    voiced, asp = rng.uniform(0.0, 1.0, (B, T)), rng.uniform(0.0, 0.3, (B, T))
    s64, status, cycles = R.source(f0, voiced, asp, frames, S, fs, seed=3)
    sl, _, _ = R.source(f0, voiced, asp, frames, S, fs, seed=3, dtype=np.longdouble)
    got, got_status = launch_source(dev, f0, voiced, asp, np.array(frames), S, fs, seed=3, pitch=T * S + 5)
    assert np.array_equal(got_status, status) and (status == 0).all()
    floor = 2.0 ** -52 * (1 + cycles) * np.pi / (2 * R.FALL)
    assert_parity(got[:, :T * S], s64, sl, floor, f"source {case}")
    for b in range(B):
        assert (got[b, frames[b] * S:] == 0).all()


def test_noise_is_exact(dev):
    """voiced_amp = 0, asp_amp = 1: the source is nu(seed, 0, b, n) itself, bit for bit; another seed gives other values."""
    B, T, S = 3, 5, 33
    one, zero = np.ones((B, T)), np.zeros((B, T))
    got, _ = launch_source(dev, 100.0 * one, zero, one, np.full(B, T), S, 1650.0, seed=(1 << 63) + 12345)
    want = np.stack([R.noise((1 << 63) + 12345, 0, b, np.arange(T * S)) for b in range(B)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    other, _ = launch_source(dev, 100.0 * one, zero, one, np.full(B, T), S, 1650.0, seed=7)
    assert not np.array_equal(other, got)


def test_source_status(dev):
    """A non-finite control in a used frame: that row is NaN, bit 1; in an unused frame it is ignored."""
    B, T, S = 3, 4, 10
    f0, voiced, asp = np.full((B, T), 120.0), np.full((B, T), 0.8), np.full((B, T), 0.1)
    frames = np.array([4, 3, 4])
    clean, _ = launch_source(dev, f0, voiced, asp, frames, S, 500.0)
    voiced[0, 2] = np.nan
    f0[1, 3] = np.inf          # unused: frames[1] = 3
    got, status = launch_source(dev, f0, voiced, asp, frames, S, 500.0)
    assert status.tolist() == [2, 0, 0]
    assert np.isnan(got[0, :40]).all()
    assert np.array_equal(got[1:].view(np.uint64), clean[1:].view(np.uint64))


def small(rng, B=3, T=4, S=40, K=(5, 9, 7)):
    areas = np.exp(0.5 * rng.standard_normal((B, T, max(K))))
    src, _, _ = R.source(np.full((B, T), 150.0), np.ones((B, T)), np.full((B, T), 0.05), np.full(B, T), S, 2000.0)
    return areas, np.array(K, np.int32), np.full(B, T, np.int32), src


def test_padding_and_nothing_behind_the_pitch(dev):
    """Sentinel-filled outputs with a pitch above T S: every sample from n_b to the pitch is 0, each output alone works, and
    the guard behind the last row is untouched (launch_ladder asserts that)."""
    rng = np.random.default_rng(5)
    areas, K, frames, src = small(rng)
    frames = np.array([4, 0, 2], np.int32)
    pitch = src.shape[1] + 3
    src = np.concatenate([src, np.full((3, 3), np.nan)], 1)   # the padding of the source is never read
    both, status = launch_ladder(dev, areas, K, frames, 40, src)
    assert (status == 0).all()
    for b, n in enumerate(frames * 40):
        assert (both["out64"][b, n:pitch] == 0).all() and (both["out32"][b, n:pitch] == 0).all()
        assert (both["out64"][b, :n] != SENTINEL).all()
    assert np.abs(both["out64"][0]).max() > 0 and (both["out64"][1] == 0).all()
    only64, _ = launch_ladder(dev, areas, K, frames, 40, src, outputs=("out64",))
    only32, _ = launch_ladder(dev, areas, K, frames, 40, src, outputs=("out32",))
    assert np.array_equal(only64["out64"].view(np.uint64), both["out64"].view(np.uint64))
    assert np.array_equal(only32["out32"].view(np.uint32), both["out32"].view(np.uint32))


def test_ladder_status(dev):
    """A closure sets bit 0 and is computed as min_area; a NaN area in a used frame gives NaN for that utterance only; a NaN in
    an unused frame or section is ignored."""
    rng = np.random.default_rng(6)
    areas, K, frames, src = small(rng)
    frames = np.array([4, 4, 3], np.int32)
    clean, _ = launch_ladder(dev, areas, K, frames, 40, src)
    closed = areas.copy()
    closed[0, 1, 2] = 1e-7
    clamped = closed.copy()
    clamped[0, 1, 2] = R.MIN_AREA
    got, status = launch_ladder(dev, closed, K, frames, 40, src)
    want, _ = launch_ladder(dev, clamped, K, frames, 40, src)
    assert status.tolist() == [1, 0, 0]
    assert np.array_equal(got["out64"].view(np.uint64), want["out64"].view(np.uint64))
    ref, ref_status = R.ladder(closed, K, frames, 40, src)
    refl, _ = R.ladder(closed, K, frames, 40, src, dtype=np.longdouble)
    assert ref_status.tolist() == [1, 0, 0]
    assert_parity(got["out64"], ref, refl, K * 2.0 ** -52, "closure")
    broken = areas.copy()
    broken[1, 2, 3] = np.nan
    broken[2, 3, 0] = np.nan       # unused: frames[2] = 3
    broken[0, 0, 7] = np.inf       # unused: K_0 = 5
    got, status = launch_ladder(dev, broken, K, frames, 40, src)
    assert status.tolist() == [0, 2, 0]
    assert np.isnan(got["out64"][1, :160]).all() and np.isnan(got["out32"][1, :160]).all()
    for b in (0, 2):
        assert np.array_equal(got["out64"][b].view(np.uint64), clean["out64"][b].view(np.uint64))
    negative = areas.copy()
    negative[2, 0, 1] = -1.0
    bad_source = src.copy()
    bad_source[0, 17] = np.nan
    _, status = launch_ladder(dev, negative, K, frames, 40, bad_source)
    assert status.tolist() == [2, 0, 2]


def test_refusals_leave_the_outputs_alone(dev):
    """K = 0 and K = 65 (AS_ERR_UNSUPPORTED = -2) and an injection section outside 1 .. K - 1 (AS_ERR_BAD_ARG = -1) return their
    code before anything is launched: every output element still holds the sentinel."""
    rng = np.random.default_rng(7)
    areas = np.exp(0.5 * rng.standard_normal((2, 3, 65)))
    src = rng.standard_normal((2, 30))
    frames = np.array([3, 3], np.int32)
    where, gain = np.full((2, 3), -1, np.int32), np.full((2, 3), 0.1)
    for K, w, code in (((4, 0), None, -2), ((65, 4), None, -2), ((4, 6), (1, 1, 6), -1), ((4, 6), (0, 0, 0), -1), ((4, 6), (1, 1, 4), -1)):
        if w is not None:
            where[0] = w
        got, status = launch_ladder(dev, areas, np.array(K, np.int32), frames, 10, src, where if w is not None else None,
                                    gain if w is not None else None, expect=code)
        assert (got["out64"] == SENTINEL).all() and (got["out32"] == SENTINEL).all() and (status == -5).all()
    where[0] = (1, 3, -1)          # the range is 1 .. K_b - 1, per utterance: 3 is fine with four sections
    _, status = launch_ladder(dev, areas, np.array((4, 6), np.int32), frames, 10, src, where, gain)
    assert (status == 0).all()


def test_equal_bits_on_every_run_and_alone_or_in_a_batch(dev):
    x = reference(1)["x"]
    args = (x["areas"], x["sections"], x["frames"], x["S"], x["source"], x["where"], x["gain"], x["seed"])
    one, _ = launch_ladder(dev, *args)
    two, _ = launch_ladder(dev, *args)
    assert np.array_equal(one["out64"].view(np.uint64), two["out64"].view(np.uint64))
    # without frication every utterance alone gives its bits of the batch; with it utterance 0 does (the noise is nu(.., b, n))
    plain, _ = launch_ladder(dev, *args[:5])
    for b in range(len(x["sections"])):
        alone, _ = launch_ladder(dev, x["areas"][b:b + 1], x["sections"][b:b + 1], x["frames"][b:b + 1], x["S"], x["source"][b:b + 1])
        assert np.array_equal(alone["out64"][0].view(np.uint64), plain["out64"][b].view(np.uint64)), b
    alone, _ = launch_ladder(dev, x["areas"][:1], x["sections"][:1], x["frames"][:1], x["S"], x["source"][:1], x["where"][:1],
                             x["gain"][:1], x["seed"])
    assert np.array_equal(alone["out64"][0].view(np.uint64), one["out64"][0].view(np.uint64))


def test_uniform_tube_resonates_at_its_closed_form_on_the_device(dev):
    """The host test's closed form from the device's out64: a uniform ladder of K = 22 sections, r_g = 0.97, r_l = -0.97, mu = 1,
    no differencing; the first four peaks of the impulse response's spectrum lie at (2n - 1) fs / 4K within one FFT bin."""
    K, N, fs, nfft = 22, 8192, 44100.0, 1 << 17
    src = np.zeros((1, N))
    src[0, 0] = 1.0
    got, status = launch_ladder(dev, np.ones((1, 1, K)), np.array([K], np.int32), np.array([1], np.int32), N, src, r_g=0.97, r_l=-0.97,
                                mu=1.0, radiation=0)
    assert status.tolist() == [0]
    spectrum = np.abs(np.fft.rfft(got["out64"][0], nfft))
    peaks = [i for i in range(1, len(spectrum) - 1) if spectrum[i] > spectrum[i - 1] and spectrum[i] >= spectrum[i + 1]
             and spectrum[i] > 0.3 * spectrum.max()][:4]
    want = (2 * np.arange(1, 5) - 1) * fs / (4 * K)
    print("peaks", np.array(peaks) * fs / nfft, "closed form", want)
    assert np.abs(np.array(peaks) * fs / nfft - want).max() <= fs / nfft


def test_the_module_matches_the_restatement_on_the_glue(dev):
    """equal_sections and frication_control (torch ops on the device) against their restatement on ragged hand-made sections, and
    the wrappers against the C ABI."""
    from artspeech_amd import vocal_tract_synthesis as V
    rng = np.random.default_rng(8)
    B, T, Kr = 3, 6, 11
    areas, lengths = rng.uniform(0.05, 6.0, (B, T, Kr)), rng.uniform(0.5, 2.5, (B, T, Kr))
    counts = rng.integers(3, Kr + 1, (B, T))
    frames = np.array([6, 4, 5])
    areas[0, 0, 1] = np.nan        # the first frame takes the first valid one
    lengths[1, 2, 0] = np.inf      # a later frame takes the frame before
    counts[2, 1] = 0
    areas[0, 3, 2] = 0.01          # a constriction: frication
    fs = 16000.0
    want = R.equal_sections(areas, lengths, counts, frames, fs)
    got = V.equal_sections(on(dev, areas, np.float64), on(dev, lengths, np.float64), on(dev, counts, np.int32), on(dev, frames, np.int32), fs)
    assert np.array_equal(got.sections.cpu().numpy(), want[1]) and got.replaced.cpu().tolist() == want[3].tolist() == [1, 1, 1]
    assert np.array_equal(got.areas.cpu().numpy(), want[0])
    assert np.allclose(got.tract_length.cpu().numpy(), want[2], rtol=1e-14, atol=0)
    where, gain = V.frication_control(got.areas, got.sections, 0.3)
    want_where, want_gain = R.frication_control(want[0], want[1], 0.3)
    assert np.array_equal(where.cpu().numpy(), want_where) and (want_where >= 0).any() and (want_where < 0).any()
    assert np.allclose(gain.cpu().numpy(), want_gain, rtol=1e-14, atol=0)
    f0 = np.full((B, T), 130.0)
    src, s_status = V.glottal_source(on(dev, f0, np.float64), 0.9, 0.05, frames, 20, fs, seed=4)
    raw, _ = launch_source(dev, f0, np.full((B, T), 0.9), np.full((B, T), 0.05), frames, 20, fs, seed=4)
    assert np.array_equal(src.cpu().numpy().view(np.uint64), raw.view(np.uint64)) and (s_status == 0).all()
    out = V.waveguide(got.areas, got.sections, frames, 20, src, where, gain, seed=4)
    raw, status = launch_ladder(dev, want[0], want[1], frames, 20, raw, want_where, gain.cpu().numpy(), seed=4)
    assert np.array_equal(out.out64.cpu().numpy().view(np.uint64), raw["out64"].view(np.uint64))
    assert np.array_equal(out.out32.cpu().numpy().view(np.uint32), raw["out32"].view(np.uint32))
    assert np.array_equal(out.status.cpu().numpy(), status)
    with pytest.raises(RuntimeError, match="as_vt_waveguide failed"):
        V.waveguide(got.areas, np.array([0, 2, 2]), frames, 20, src)


def test_walls_that_touch_are_a_closure_for_synthesize_speech(dev):
    """The area function gives exactly 0 where the walls touch; synthesize_speech reads that as a closure (STATUS_CLOSED, finite
    samples, equal to the same tube with half the closure threshold there), while waveguide itself reports a 0 as a defect.
    Eight sections of 2 cm at 17.5 kHz are eight slices of c / fs: every section, the closed one included, is a slice."""
    from artspeech_amd import vocal_tract_synthesis as V
    rng = np.random.default_rng(9)
    B, T, Kr = 2, 5, 8
    areas, lengths = rng.uniform(0.5, 4.0, (B, T, Kr)), np.full((B, T, Kr), 2.0)
    areas[0, 2, 3] = 0.0
    counts, frames, voicing = np.full((B, T), Kr), np.array([T, T]), np.ones((B, T))
    args = [on(dev, lengths, np.float64), on(dev, counts, np.int32), on(dev, voicing, np.float64), on(dev, frames, np.int32), 350, 50]
    wave = V.synthesize_speech(on(dev, areas, np.float64), *args)
    assert wave.status.tolist() == [V.STATUS_CLOSED, 0] and bool(torch.isfinite(wave.samples).all()) and wave.sample_rate == 17500.0
    assert float(wave.samples[0].abs().max()) > 0 and wave.n_samples.tolist() == [1750, 1750] and wave.sections.tolist() == [8, 8]
    areas[0, 2, 3] = 0.5 * V.MIN_AREA
    same = V.synthesize_speech(on(dev, areas, np.float64), *args)
    assert torch.equal(same.samples, wave.samples)
    eq = V.equal_sections(on(dev, np.where(areas == 0.5 * V.MIN_AREA, 0.0, areas), np.float64), args[0], args[1], args[3], 17500.0)
    assert float(eq.areas[0, 2, 3]) == 0.0
    src, _ = V.glottal_source(torch.full((B, T), 100.0, dtype=torch.float64, device=dev), 1.0, 0.0, frames, 350, 17500.0)
    assert V.waveguide(eq.areas, eq.sections, frames, 350, src).status.tolist() == [V.STATUS_NON_FINITE, 0]


def test_from_a_tree_of_air_columns_to_log_mel_features(dev, tmp_path):
    """End to end: a hand-made tree of two sequences of six frames -> vocal_tract_speech.main -> speech.wav reads back,
    the manifest feeds RecordedAcousticRecognitionDataset, acoustic_collate_fn gives finite log-mel features."""
    import yaml

    import vocal_tract_speech
    from artspeech_amd.phoneme_recognition.datasets import RecordedAcousticRecognitionDataset, acoustic_collate_fn, read_wav
    from artspeech_amd.phoneme_recognition.features import MelSpectrogram
    from conftest import ROOT
    with open(os.path.join(ROOT, "configs", "vocal_tract_speech_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    phi = np.linspace(0.0, 2 * np.pi, 100)
    phonemes = [["a", "a", "s", "s", "a", "#"], ["#", "a", "a", "a", "t", "t"]]
    gaps = {"a": 0.04, "s": 0.008, "t": 0.02, "#": 0.03}   # walls that are circles round the grid's centre, as the formants' test has
    for s, tokens in enumerate(phonemes):
        seq = tmp_path / "subject" / f"S{s}"
        (seq / "air_column").mkdir(parents=True)
        (seq / "target_sequence.txt").write_text(" ".join(tokens))
        for t, token in enumerate(tokens):
            r_int = 0.12 + 0.01 * t + 0.02 * s
            walls = [np.stack([0.5 + r * np.cos(phi), 0.5 + r * np.sin(phi)]) for r in (r_int, r_int + gaps[token])]
            np.save(seq / "air_column" / f"{t:04d}.npy", np.stack(walls))
    cfg.update(datadir=str(tmp_path), sample_rate=16000, model_sample_rate=None, voiced_tokens=["a"])
    report = vocal_tract_speech.main(**cfg)
    assert report["samples_per_frame"] == 320 and report["sample_rate"] == 16000 and len(report["sequences"]) == 2
    for s, entry in enumerate(report["sequences"]):
        wav, rate = read_wav(tmp_path / "subject" / f"S{s}" / "speech.wav")
        assert rate == 16000 and wav.dtype == torch.int16 and len(wav) == 6 * 320 == entry["samples"]
        assert int(wav.abs().max()) > 1000 and not entry["status"]["non_finite"] and 2 <= entry["sections"] <= 64
        with open(tmp_path / "subject" / f"S{s}" / "speech.json") as f:
            assert json.load(f)["sections"] == entry["sections"]
    vocabulary = {"<unk>": 0, "#": 1, "a": 2, "s": 3, "t": 4}
    ds = RecordedAcousticRecognitionDataset(str(tmp_path / "manifest.json"), vocabulary, framerate=50, voiced_tokens=["a"])
    assert len(ds) == 2
    items = [ds[0], ds[1]]
    assert items[0]["phonemes_with_time"] == [("a", 0.0, 0.04), ("s", 0.04, 0.08), ("a", 0.08, 0.1), ("#", 0.1, 0.12)]
    assert items[1]["articulatory_target"].tolist() == [1, 2, 2, 2, 4, 4]
    mel = MelSpectrogram(sample_rate=16000, n_fft=256, win_length=256, hop_length=64, n_mels=20)
    batch = acoustic_collate_fn(items, mel, device=dev)
    feats = batch["melspec"]
    assert feats.shape[:3] == (2, 2, 20) and feats.shape[3] == int(batch["melspec_length"].max()) and bool(torch.isfinite(feats).all())
