"""Host-side pieces of the vocal-tract acoustics (no GPU): the restatement of tests/vt_acoustics_fp64.py against the closed forms
its definition has and the properties it promises, the inputs that the device tests draw, the library's argument checks, the
Python layer's refusal of CPU tensors and the script's config."""
import inspect
import os

import numpy as np
import pytest
import torch

import vt_acoustics_fp64 as R
from conftest import ROOT

C = R.C_SOUND
WIDTH = R.bracket_width(10.0, 3)   # 5.83e-4 Hz


def uniform_tube(L=17.5, area=5.0, K=35):
    return np.full((1, K), area), np.full((1, K), L / K)


def two_tubes():
    areas = np.concatenate([np.full((1, 16), 1.0), np.full((1, 19), 8.0)], axis=1)
    lengths = np.concatenate([np.full((1, 16), 8.0 / 16), np.full((1, 19), 9.5 / 19)], axis=1)
    return areas, lengths


# ---------------------------------------------------------------------------------------------------- the restatement
def test_uniform_tube_resonates_at_odd_quarter_wavelengths():
    areas, lengths = uniform_tube()
    freq, level, found, status = R.formants(areas, lengths, radiation=0, f0=10.0, df=10.0, F=500, n_formants=5, rounds=3)
    want = (2 * np.arange(1, 6) - 1) * C / (4 * 17.5)
    assert want.tolist() == [500, 1500, 2500, 3500, 4500] and found.tolist() == [5] and status.tolist() == [0]
    print("uniform tube:", freq[0], "off by", np.abs(freq[0] - want).max())
    assert np.abs(freq[0] - want).max() <= WIDTH
    assert abs(WIDTH - 5.83e-4) < 1e-6


def test_piston_lowers_the_first_formant_by_the_end_correction():
    areas, lengths = uniform_tube()
    f1 = R.formants(areas, lengths, radiation=1)[0][0, 0]
    a = np.sqrt(5.0 / np.pi)
    low, high, corrected = C / (4 * (17.5 + a)), C / (4 * 17.5), C / (4 * (17.5 + 8 * a / (3 * np.pi)))
    print(f"piston: F1 = {f1:.4f}, c / 4(L + a) = {low:.2f}, c / 4(L + 8a / 3 pi) = {corrected:.2f}")
    assert abs(low - 466.38) < 0.01 and abs(corrected - 471.17) < 0.01
    assert low < f1 < high and abs(f1 - corrected) <= 1e-3 * corrected


def test_two_tubes_against_the_roots_of_their_closed_form():
    roots = R.two_tube_roots()
    assert np.abs(roots - [775.238, 1237.175, 2697.515, 3339.192, 4582.735]).max() < 1e-3
    freq, _, found, _ = R.formants(*two_tubes(), radiation=0)
    print("two tubes:", freq[0], "roots", roots)
    assert found.tolist() == [5] and np.abs(freq[0] - roots).max() <= WIDTH


def test_chain_matrices_have_unit_determinant():
    """|A D - B C - 1| <= 1e-12.  A D and B C cancel, so the determinant carries the rounding of K products at the scale
    |A D| + |B C|: the chains are drawn with areas in 1 .. 3 cm^2, where K eps (|A D| + |B C|) stays below the bound (asserted)."""
    rng = np.random.default_rng(0)
    for K in (1, 7, 35, 99):
        _, lengths = R.draw(rng, 6, K)
        areas = np.exp(rng.uniform(0.0, np.log(3.0), (6, K)))
        f = np.broadcast_to(R.frequency_grid(10.0, 10.0, 500), (6, 500))
        A, B, Cc, D = R.chain(f, areas, lengths, np.full(6, K))
        assert K * 2.0 ** -52 * (np.abs(A * D) + np.abs(B * Cc)).max() <= 1e-12
        assert np.abs(A * D - B * Cc - 1).max() <= 1e-12
        assert np.abs(A.imag).max() == 0 and np.abs(D.imag).max() == 0 and np.abs(B.real).max() == 0 and np.abs(Cc.real).max() == 0


def test_cutting_any_section_in_two_halves_leaves_den_alone():
    rng = np.random.default_rng(1)
    _, lengths = R.draw(rng, 1, 9)
    areas = np.exp(rng.uniform(0.0, np.log(3.0), (1, 9)))   # |den| of order one, as for the determinant: the bound is absolute
    for radiation in (0, 1):
        want = R.transfer(areas, lengths, radiation=radiation)[0]
        for i in range(9):
            a2 = np.insert(areas, i, areas[0, i], axis=1)
            l2 = np.insert(lengths, i, lengths[0, i] / 2, axis=1)
            l2[0, i + 1] = lengths[0, i] / 2
            got = R.transfer(a2, l2, radiation=radiation)[0]
            assert np.abs(got - want).max() <= 1e-12, (radiation, i)


def test_scaling_all_areas_leaves_the_open_end_formants_alone():
    rng = np.random.default_rng(2)
    areas, lengths = R.draw(rng, 4, 35)
    want = R.formants(areas, lengths, radiation=0)
    for scale in (0.25, 3.0):
        got = R.formants(areas * scale, lengths, radiation=0)
        assert np.array_equal(got[2], want[2]) and np.nanmax(np.abs(got[0] - want[0])) <= WIDTH


def test_status_bits_and_nan_fill():
    rng = np.random.default_rng(3)
    areas, lengths = R.draw(rng, 7, 12)
    counts = np.array([12, 12, 12, 12, 12, 0, 5])
    areas[1, 4] = 0.0              # a closure
    areas[2, 7] = np.nan
    lengths[3, 0] = -0.5
    lengths[4, 11] = np.inf
    areas[6, 8] = np.nan           # behind the frame's count: not looked at
    freq, level, found, status = R.formants(areas, lengths, counts)
    den, H, status_t = R.transfer(areas, lengths, counts)
    assert status.tolist() == status_t.tolist() == [0, R.STATUS_CLOSED, 2, 2, 2, 2, 0]
    assert (R.STATUS_CLOSED, R.STATUS_NON_FINITE) == (1, 2)
    bad = status == R.STATUS_NON_FINITE
    assert np.isnan(freq[bad]).all() and np.isnan(level[bad]).all() and (found[bad] == 0).all()
    assert np.isnan(den[bad]).all() and np.isnan(H[bad]).all()
    assert np.isfinite(den[~bad]).all() and np.isfinite(H[~bad]).all() and (found[~bad] > 0).all()
    clamped = areas.copy()
    clamped[1, 4] = R.MIN_AREA
    assert np.array_equal(R.transfer(clamped, lengths, counts)[0][1], den[1])          # computed as min_area
    assert np.array_equal(R.transfer(areas[:, :5], lengths[:, :5])[0][6], den[6])      # the first counts[n] sections


def test_fewer_minima_than_formants_asked_for():
    areas, lengths = uniform_tube()
    freq, level, found, _ = R.formants(areas, lengths, radiation=0, n_formants=8)
    assert found.tolist() == [5] and np.isnan(freq[0, 5:]).all() and np.isnan(level[0, 5:]).all() and np.isfinite(freq[0, :5]).all()
    freq, _, found, _ = R.formants(areas, lengths, radiation=0, n_formants=0)
    assert freq.shape == (1, 0) and found.tolist() == [0]
    freq, _, found, _ = R.formants(areas, lengths, radiation=0, f0=490.0, df=10.0, F=3, n_formants=2, rounds=0)   # bin 1 = bin F-2
    assert found.tolist() == [1] and freq[0, 0] == 500.0


def test_the_device_tests_inputs_stay_within_the_redraw_cap():
    """The draws of tests/test_gpu_vt_acoustics.py, checked here on the CPU: at most 2 % of a case's frames are drawn again."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    for case in R.CASES:
        x = R.draw_case(case)
        assert x["redrawn"] <= R.MAX_REDRAWN * case[0], (case, x["redrawn"])
        prepared, used, status = R.prepare(x["areas"], x["lengths"], x["counts"])
        g = R.power(R.denominator(np.broadcast_to(R.frequency_grid(x["f0"], x["df"], x["F"]), (case[0], x["F"])), prepared, x["lengths"],
                                  used, x["radiation"]))
        assert R.strict(g).all() and (status == 0).all()
    assert {c[1] for c in R.CASES} >= {1, 2, 35, 99, 1024} and {c[2] for c in R.CASES} >= {3, 63, 64, 65, 255, 256, 257, 500, 4096}
    assert {c[0] for c in R.CASES} == {1, 2, 37} and {c[3] for c in R.CASES} == {0, 1, 5, 8} and {c[4] for c in R.CASES} == {0, 1, 3, 6}


def test_the_cases_ask_no_more_rounds_than_float64_can_rank():
    """The reference's own error decides how many rounds a case may ask for: the restatement in float64 and in longdouble must
    agree on every formant of a case within a quarter of the last bracket.  Six rounds with the piston do not: the smooth
    minimum of g leaves the probes of the last rounds equal to the last bit (the figures are printed)."""
    for case in R.CASES:
        if case[1] > 99:
            continue   # K = 1024 asks for three rounds at the open end, as K = 35 does; its longdouble chain takes seconds
        x = R.draw_case(case)
        kw = dict(f0=x["f0"], df=x["df"], F=x["F"], radiation=x["radiation"], n_formants=x["n_formants"], rounds=x["rounds"])
        f64 = R.formants(x["areas"], x["lengths"], x["counts"], **kw)
        wide = R.formants(x["areas"], x["lengths"], x["counts"], dtype=np.longdouble, **kw)
        assert np.array_equal(f64[2], wide[2]), case
        if f64[2].sum():
            assert np.nanmax(np.abs(f64[0] - wide[0])) <= 0.25 * R.bracket_width(x["df"], x["rounds"]), case
    areas, lengths = uniform_tube()
    for rounds in (3, 6):
        a = R.formants(areas, lengths, radiation=1, rounds=rounds)[0]
        b = R.formants(areas, lengths, radiation=1, rounds=rounds, dtype=np.longdouble)[0]
        print(f"piston, {rounds} rounds: float64 and longdouble differ by {np.abs(a - b).max():.3e} Hz, bracket {R.bracket_width(10.0, rounds):.3e}")


# ---------------------------------------------------------------------------------------------------- the library
def _call(**change):
    from artspeech_amd import _lib
    a = dict(frames=4, K=35, f0=10.0, df=10.0, F=500, radiation=1, c=R.C_SOUND, rho=R.RHO, min_area=R.MIN_AREA, n_formants=5,
             rounds=3, areas=16, lengths=16, den=16, transfer=16)
    a.update(change)
    _lib.call("as_vt_acoustics", a["areas"], a["K"], 1, a["lengths"], a["K"], 1, None, a["frames"], a["K"], a["f0"], a["df"], a["F"],
              a["radiation"], a["c"], a["rho"], a["min_area"], a["n_formants"], a["rounds"], a["den"], a["transfer"], 16, 16, 16, 16,
              stream=0)


def test_limits_are_refused_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail otherwise (or crash); these return the library's message."""
    bad = [dict(K=0), dict(K=1025), dict(F=2), dict(F=4097), dict(n_formants=-1), dict(n_formants=9), dict(rounds=-1), dict(rounds=7),
           dict(frames=-1), dict(f0=0.0), dict(df=0.0), dict(df=float("nan")), dict(radiation=2), dict(c=0.0), dict(rho=-1.0),
           dict(min_area=0.0), dict(areas=None), dict(lengths=None), dict(den=8)]
    for change in bad:
        with pytest.raises(RuntimeError, match="as_vt_acoustics failed"):
            _call(**change)
    with pytest.raises(RuntimeError, match=r"1025 sections \(1 \.\. 1024 supported\)"):
        _call(K=1025)
    with pytest.raises(RuntimeError, match=r"2 frequency bins \(3 \.\. 4096 supported\)"):
        _call(F=2)
    _call(frames=0)                                      # nothing to do: no launch, no error
    _call(frames=0, K=1, F=3, n_formants=0, rounds=0)    # the limits themselves are inside
    _call(frames=0, K=1024, F=4096, n_formants=8, rounds=6, den=None, transfer=None)


def test_symbol_is_declared_bound_and_built():
    from artspeech_amd import _lib, build
    L = _lib.lib()
    assert "as_vt_acoustics" in _lib.PROTOTYPES and hasattr(L, "as_vt_acoustics")
    res, args = _lib.PROTOTYPES["as_vt_acoustics"]
    assert len(args) == 25 and args[-1] is _lib.Stream and res is _lib.C.c_int32
    assert all(a is _lib.C.c_void_p for a in args[-7:-1])          # den, transfer, freq, level, found, status
    assert "vt_acoustics.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    source = open(os.path.join(build.CSRC, "vt_acoustics.hip")).read()
    assert "int as_vt_acoustics(" in header and "double* den, double* transfer, double* freq" in header
    for text in (header, source):
        for word in ("ASSUMPTION", "unpinned", "(2n - 1) c / 4L"):
            assert word in text, word
    assert "getenv" not in source


def test_python_layer_refuses_cpu_tensors_and_exports_the_status_bits():
    from artspeech_amd import vocal_tract_acoustics as V
    assert (V.STATUS_CLOSED, V.STATUS_NON_FINITE) == (R.STATUS_CLOSED, R.STATUS_NON_FINITE) == (1, 2)
    assert (V.SOUND_SPEED, V.AIR_DENSITY, V.MIN_AREA) == (R.C_SOUND, R.RHO, R.MIN_AREA) == (35000.0, 1.14e-3, 1e-4)
    assert V.Formants._fields == ("frequencies", "levels", "found", "status")
    areas, lengths = (torch.from_numpy(t) for t in uniform_tube())
    for fn in (V.transfer_function, V.formants):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(areas, lengths)
        p = inspect.signature(fn).parameters
        assert (p["f0"].default, p["df"].default, p["n_freq"].default, p["radiation"].default) == (10.0, 10.0, 500, "piston")
    with pytest.raises(RuntimeError, match="MI355X"):
        V.tube_sections(torch.zeros(3, 5), torch.zeros(3, 5), 22.0)
    p = inspect.signature(V.formants).parameters
    assert (p["n_formants"].default, p["rounds"].default) == (5, 3)
    with pytest.raises(ValueError, match="radiation"):
        V.formants(areas, lengths, radiation="horn")


def test_script_config_keys_are_main_parameters():
    import yaml
    import vocal_tract_formants as S
    from artspeech_amd.area_function import build_semipolar_grid
    assert not S.__name__.startswith(("train_", "test_"))
    with open(os.path.join(ROOT, "configs", "vocal_tract_formants_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= set(inspect.signature(S.main).parameters)
    assert set(cfg["grid"]) <= set(inspect.signature(build_semipolar_grid).parameters)
    grid = build_semipolar_grid(**cfg["grid"])
    assert grid.ndim == 3 and grid.shape[1:] == (cfg["grid"]["grid_res"], 2) and 2 <= grid.shape[0] <= R.MAX_K
    with open(os.path.join(ROOT, "configs", "generate_vocal_tract_shape_air_column_synthetic.yaml")) as f:
        gen = yaml.safe_load(f)
    assert cfg["datadir"] == os.path.dirname(gen["save_to"]) and cfg["database_name"] == gen["database_name"]
