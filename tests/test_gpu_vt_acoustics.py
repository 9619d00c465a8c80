"""as_vt_acoustics on the device against the numpy restatement (tests/vt_acoustics_fp64.py).

den and transfer.  Per frame the yardstick is measured, not fixed: e64 = max over the bins of |restatement in float64 -
restatement in longdouble| divided by the frame's max |den|.  The device must stay within 16 max(e64, K 2^-52) of the longdouble
restatement by the same norm: its sine, cosine and contraction choices are another rounding path of the same length, not a less
accurate one -- hence a constant factor, not a new scale.  The transfer function is compared where |den| exceeds 1e-6 of the
frame's maximum, and in the same norm: H = 1 / den exactly, so 1 / H of the device is held against the restatement's den (below
that threshold the inversion would amplify the rounding of H itself past the yardstick).

Formants.  The same ``found``; every frequency within the last bracket's width 2 df (2 / 65)^R; levels within 1e-6 dB where g at
the formant exceeds 1e-12.  The inputs are drawn so that, on the restatement alone, every coarse minimum is strict by a relative
1e-9 on both sides (vt_acoustics_fp64.strict; at most 2 % of a case's frames are drawn again, which the host tests check for the
same seeds): rounding cannot change the set of minima."""
import json
import os

import numpy as np
import pytest
import torch

import vt_acoustics_fp64 as R

pytestmark = pytest.mark.gpu

OUTPUTS = ("den", "transfer", "freq", "level", "found", "status")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def launch(dev, areas, lengths, counts=None, f0=10.0, df=10.0, F=500, radiation=1, n_formants=5, rounds=3, c=R.C_SOUND, rho=R.RHO,
           min_area=R.MIN_AREA, outputs=OUTPUTS):
    """The C ABI as it is: contiguous (n, K) inputs, every output in ``outputs`` allocated (and filled with a sentinel first, so
    that an element the kernel left alone shows), the others NULL.  Returns {name: numpy array}."""
    from artspeech_amd import _lib
    a = torch.from_numpy(np.ascontiguousarray(areas, np.float64)).to(dev)
    l = torch.from_numpy(np.ascontiguousarray(lengths, np.float64)).to(dev)
    n, K = a.shape
    cnt = None if counts is None else torch.from_numpy(np.asarray(counts, np.int32)).to(dev)
    shapes = {"den": ((n, F), torch.complex128), "transfer": ((n, F), torch.complex128), "freq": ((n, n_formants), torch.float64),
              "level": ((n, n_formants), torch.float64), "found": ((n,), torch.int32), "status": ((n,), torch.int32)}
    out = {}
    for name, (shape, dtype) in shapes.items():
        out[name] = torch.full(shape, -77, dtype=dtype, device=dev) if name in outputs else None
    _lib.call("as_vt_acoustics", a, K, 1, l, K, 1, cnt, n, K, float(f0), float(df), F, radiation, c, rho, min_area, n_formants, rounds,
              *[out[name] for name in OUTPUTS])
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items() if t is not None}


_REFERENCES = {}


def reference(case):
    """The restatement of one of R.CASES, computed once and shared by the tests that read it."""
    if case not in _REFERENCES:
        x = R.draw_case(case)
        grid = dict(f0=x["f0"], df=x["df"], F=x["F"], radiation=x["radiation"])
        d64, h64, status = R.transfer(x["areas"], x["lengths"], x["counts"], **grid)
        dl, hl, _ = R.transfer(x["areas"], x["lengths"], x["counts"], dtype=np.longdouble, **grid)
        fm = R.formants(x["areas"], x["lengths"], x["counts"], n_formants=x["n_formants"], rounds=x["rounds"], **grid)
        _REFERENCES[case] = dict(x=x, grid=grid, d64=d64, dl=dl, formants=fm, status=status)
    return _REFERENCES[case]


def assert_den_parity(got_den, got_h, d64, dl, K, what):
    scale = np.abs(dl).max(1)
    e64 = (np.abs(d64 - dl).max(1) / scale).astype(np.float64)
    tol = 16 * np.maximum(e64, K * 2.0 ** -52)
    err = (np.abs(got_den - dl).max(1) / scale).astype(np.float64)
    with np.errstate(all="ignore"):
        back = 1 / got_h.astype(np.clongdouble)
    compared = np.abs(dl) > 1e-6 * scale[:, None]
    err_h = (np.where(compared, np.abs(back - dl), 0).max(1) / scale).astype(np.float64)
    print(f"{what}: den error / yardstick {np.max(err / tol):.3f} (error {err.max():.2e}, e64 {e64.max():.2e}), "
          f"transfer {np.max(err_h / tol):.3f} on {int(compared.sum())} of {compared.size} bins")
    assert (err <= tol).all(), what
    assert (err_h <= tol).all(), what
    return float(np.max(err / tol))


def assert_formant_parity(got, ref, df, rounds, what):
    freq, level, found, status = ref
    assert np.array_equal(got["status"], status), what
    assert np.array_equal(got["found"], found), what
    have = np.arange(freq.shape[1])[None, :] < found[:, None]
    assert np.isnan(got["freq"][~have]).all() and np.isnan(got["level"][~have]).all(), what
    width = R.bracket_width(df, rounds)
    err = np.abs(got["freq"][have] - freq[have])
    g = 10.0 ** (-level[have] / 10.0)
    err_level = np.abs(got["level"][have] - level[have])[g > 1e-12]
    print(f"{what}: {int(have.sum())} formants, max |frequency error| {err.max() if err.size else 0:.3e} Hz (bracket {width:.3e}), "
          f"max |level error| {err_level.max() if err_level.size else 0:.3e} dB on {err_level.size} levels")
    assert (err <= width).all(), what
    assert (err_level <= 1e-6).all(), what


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "n{}-K{}-F{}-nf{}-R{}-rad{}-{}".format(*c[:6], "ragged" if c[6] else "full"))
def test_against_the_restatement(dev, case):
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "longdouble is no wider than float64 on this machine"
    ref = reference(case)
    x = ref["x"]
    assert x["redrawn"] <= R.MAX_REDRAWN * case[0]
    got = launch(dev, x["areas"], x["lengths"], x["counts"], n_formants=x["n_formants"], rounds=x["rounds"], **ref["grid"])
    assert (got["status"] == 0).all()
    assert_den_parity(got["den"], got["transfer"], ref["d64"], ref["dl"], case[1], f"case {case}")
    assert_formant_parity(got, ref["formants"], x["df"], x["rounds"], f"case {case}")


def test_the_cases_hold_short_frames_and_both_section_walks():
    """What the parametrised cases are meant to contain: frames with fewer minima than asked for, a frame of one section and of
    all K, and frames of equal lengths beside unequal ones in one batch."""
    fewer = ragged_ends = 0
    for case in R.CASES:
        ref = reference(case)
        x, found = ref["x"], ref["formants"][2]
        fewer += int((found < x["n_formants"]).sum())
        if x["counts"] is not None and case[1] < 1024:
            ragged_ends += int(x["counts"][0] == case[1] and x["counts"][-1] == 1)
        if case[0] > 1:
            equal = (x["lengths"] == x["lengths"][:, :1]).all(1)
            assert equal.any() and not equal.all(), case
    assert fewer >= 10 and ragged_ends >= 3


def test_minima_at_the_first_and_the_last_bin_that_can_hold_one(dev):
    """Uniform tubes whose first resonance c / 4L sits exactly on bin 1 (frame 0) and on bin F-2 (frame 1), for an F of one step
    of the minimum scan, of two, and F = 3 where bin 1 is bin F-2."""
    for F in (3, 64, 66, 130):
        f0, df = 490.0, 10.0
        targets = np.array([f0 + df, f0 + (F - 2) * df])
        K = 7
        lengths = np.repeat((R.C_SOUND / (4 * targets) / K)[:, None], K, axis=1)
        areas = np.full((2, K), 3.0)
        want = R.formants(areas, lengths, f0=f0, df=df, F=F, radiation=0, n_formants=8, rounds=3, return_bins=True)
        rows, slots, bins = want[5]
        assert bins[rows == 0][0] == 1 and bins[rows == 1][-1] == F - 2 and R.strict(want[4]).all()
        got = launch(dev, areas, lengths, f0=f0, df=df, F=F, radiation=0, n_formants=8, rounds=3)
        assert_formant_parity(got, want[:4], df, 3, f"ends, F = {F}")
        assert abs(got["freq"][0, 0] - targets[0]) <= R.bracket_width(df, 3)
        assert abs(got["freq"][1, want[2][1] - 1] - targets[1]) <= R.bracket_width(df, 3)


def special_batch():
    rng = np.random.default_rng(11)
    areas, lengths = R.draw(rng, 9, 35)
    counts = np.full(9, 35)
    areas[1, 20] = 0.0            # a closure
    areas[3, 34] = np.nan
    lengths[5, 0] = -0.25
    counts[7] = 0
    return areas, lengths, counts


def test_closure_and_bad_frames_between_good_ones(dev):
    areas, lengths, counts = special_batch()
    got = launch(dev, areas, lengths, counts)
    assert got["status"].tolist() == [0, R.STATUS_CLOSED, 0, 2, 0, 2, 0, 2, 0]
    bad = got["status"] == R.STATUS_NON_FINITE
    for name in ("den", "transfer", "freq", "level"):
        assert np.isnan(got[name][bad]).all() and np.isfinite(got[name][~bad & (np.arange(9) != 1)][:, :3]).all(), name
    assert (got["found"][bad] == 0).all()
    # the closure frame: finite, and the restatement's values at min_area
    clamped = areas.copy()
    clamped[1, 20] = R.MIN_AREA
    good = ~bad
    d64, _, status = R.transfer(clamped[good], lengths[good])
    dl = R.transfer(clamped[good], lengths[good], dtype=np.longdouble)[0]
    assert (status == 0).all() and np.isfinite(got["den"][1]).all() and np.isfinite(got["transfer"][1]).all()
    assert_den_parity(got["den"][good], got["transfer"][good], d64, dl, 35, "closure and neighbours")
    want = R.formants(areas[good], lengths[good], return_bins=True)
    assert R.strict(want[4]).all() and want[3].tolist() == [0, R.STATUS_CLOSED, 0, 0, 0, 0]
    assert_formant_parity({k: v[good] for k, v in got.items()}, want[:4], 10.0, 3, "closure and neighbours")
    # the neighbours are untouched: equal bits with the good frames run on their own
    alone = launch(dev, areas[good], lengths[good], counts[good])
    for name in OUTPUTS:
        assert np.array_equal(got[name][good], alone[name], equal_nan=True), name


def test_each_output_pointer_absent_in_turn_and_two_runs_give_equal_bits(dev):
    x = reference(R.CASES[4])["x"]   # 37 frames, K = 35, F = 255
    kw = dict(f0=x["f0"], df=x["df"], F=x["F"], radiation=x["radiation"], n_formants=5, rounds=3)
    full = launch(dev, x["areas"], x["lengths"], **kw)
    again = launch(dev, x["areas"], x["lengths"], **kw)
    for name in OUTPUTS:
        assert np.array_equal(full[name], again[name], equal_nan=True), name
        assert not (full[name] == -77).any(), name            # every element was written
    for absent in OUTPUTS:
        part = launch(dev, x["areas"], x["lengths"], outputs=[o for o in OUTPUTS if o != absent], **kw)
        assert sorted(part) == sorted(o for o in OUTPUTS if o != absent)
        for name in part:
            assert np.array_equal(part[name], full[name], equal_nan=True), (absent, name)
    none = launch(dev, x["areas"], x["lengths"], outputs=(), **kw)
    assert none == {}


def test_python_layer_strides_batch_dimensions_and_counts(dev):
    from artspeech_amd import vocal_tract_acoustics as V
    rng = np.random.default_rng(5)
    areas, lengths = R.draw(rng, 12, 35)
    counts = rng.integers(1, 36, 12)
    want = launch(dev, areas, lengths, counts)
    wide = torch.zeros(3, 4, 70, dtype=torch.float64, device=dev)
    wide[..., ::2] = torch.from_numpy(areas).to(dev).view(3, 4, 35)
    a = wide[..., ::2]                                                  # section stride 2
    l = torch.from_numpy(lengths).to(dev).view(3, 4, 35).transpose(0, 1).contiguous().transpose(0, 1)   # no single frame stride
    assert not a.is_contiguous() and not l.is_contiguous()
    fm = V.formants(a, l, torch.from_numpy(counts).view(3, 4))
    assert isinstance(fm, V.Formants) and fm.frequencies.shape == (3, 4, 5) and fm.found.shape == (3, 4) and fm.found.dtype == torch.int32
    H, status, den = V.transfer_function(a, l, counts.reshape(3, 4), return_denominator=True)
    assert H.shape == (3, 4, 500) and H.dtype == torch.complex128 and status.shape == (3, 4)
    for got, name in ((fm.frequencies, "freq"), (fm.levels, "level"), (fm.found, "found"), (fm.status, "status"), (H, "transfer"),
                      (den, "den"), (status, "status")):
        assert np.array_equal(got.cpu().numpy().reshape(want[name].shape), want[name], equal_nan=True), name
    # one row of lengths for every frame, float32 inputs, the open end by name
    row = torch.full((35,), 0.5, dtype=torch.float64, device=dev)
    got = V.formants(a.float(), row, radiation="open", n_formants=3, rounds=1)
    ref = launch(dev, a.float().double().cpu().numpy().reshape(12, 35), np.full((12, 35), 0.5), radiation=0, n_formants=3, rounds=1)
    assert np.array_equal(got.frequencies.cpu().numpy().reshape(12, 3), ref["freq"], equal_nan=True)
    over = counts.copy()
    over[::3] += 35                                                      # a count above K reads K
    got = V.formants(a, l, over.reshape(3, 4)).frequencies.cpu().numpy()
    assert np.array_equal(got.reshape(12, 5), launch(dev, areas, lengths, np.minimum(over, 35))["freq"], equal_nan=True)
    empty = V.formants(a[:0], l[:0])
    assert empty.frequencies.shape == (0, 4, 5) and empty.found.shape == (0, 4)
    areas_s, lengths_s = V.tube_sections(torch.tensor([[0.0, 0.1, 0.3]], dtype=torch.float64, device=dev),
                                         torch.tensor([[1.0, 2.0, 4.0]], dtype=torch.float64, device=dev), 10.0)
    assert torch.equal(areas_s.cpu(), torch.tensor([[150.0, 300.0]], dtype=torch.float64))
    assert torch.allclose(lengths_s.cpu(), torch.tensor([[1.0, 2.0]], dtype=torch.float64), rtol=1e-15, atol=0)
    with pytest.raises(RuntimeError, match="MI355X"):
        V.formants(a.cpu(), l)
    with pytest.raises(RuntimeError, match="1025 sections"):
        V.formants(torch.ones(2, 1025, dtype=torch.float64, device=dev), torch.ones(2, 1025, dtype=torch.float64, device=dev))


def test_closed_forms_from_the_device(dev):
    from artspeech_amd import vocal_tract_acoustics as V
    width = R.bracket_width(10.0, 3)
    areas = torch.full((1, 35), 5.0, dtype=torch.float64, device=dev)
    lengths = torch.full((1, 35), 17.5 / 35, dtype=torch.float64, device=dev)
    fm = V.formants(areas, lengths, radiation="open")
    got = fm.frequencies.cpu().numpy()[0]
    print("uniform tube:", got)
    assert fm.found.tolist() == [5] and np.abs(got - [500, 1500, 2500, 3500, 4500]).max() <= width
    f1 = float(V.formants(areas, lengths, radiation="piston").frequencies[0, 0])
    a = np.sqrt(5.0 / np.pi)
    corrected = R.C_SOUND / (4 * (17.5 + 8 * a / (3 * np.pi)))
    print("piston: F1 =", f1)
    assert R.C_SOUND / (4 * (17.5 + a)) < f1 < R.C_SOUND / (4 * 17.5) and abs(f1 - corrected) <= 1e-3 * corrected
    areas = torch.cat([torch.full((1, 16), 1.0), torch.full((1, 19), 8.0)], dim=1).double().to(dev)
    lengths = torch.cat([torch.full((1, 16), 8.0 / 16), torch.full((1, 19), 9.5 / 19)], dim=1).double().to(dev)
    got = V.formants(areas, lengths, radiation="open").frequencies.cpu().numpy()[0]
    print("two tubes:", got)
    assert np.abs(got - R.two_tube_roots()).max() <= width


def test_script_on_a_three_frame_tree(dev, tmp_path):
    """vocal_tract_formants.main on a tree of one sequence of three frames: walls that are circles round the grid's centre, so
    that every grid line that reaches them crosses each once; the outer lines cross nothing, and how many do differs by frame."""
    import yaml
    import vocal_tract_formants as S
    from conftest import ROOT
    with open(os.path.join(ROOT, "configs", "vocal_tract_formants_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    seq = tmp_path / "S1" / "one"
    (seq / "air_column").mkdir(parents=True)
    (tmp_path / "S1" / "no_air_column").mkdir()
    phi = np.linspace(0.0, 2 * np.pi, 100)
    for t, (r_int, r_ext) in enumerate([(0.06, 0.09), (0.12, 0.16), (0.2, 0.23)]):
        walls = [np.stack([0.5 + r * np.cos(phi), 0.5 + r * np.sin(phi)]) for r in (r_int, r_ext)]
        np.save(seq / "air_column" / f"{t + 1:04d}.npy", np.stack(walls))
    cfg.update(datadir=str(tmp_path), n_formants=4)
    info = S.main(**cfg)
    assert info["frames"] == 3 and [e["sequence"] for e in info["sequences"]] == [os.path.join("S1", "one")]
    freq, level = np.load(seq / "formants.npy"), np.load(seq / "formant_levels.npy")
    assert freq.shape == level.shape == (3, 4) and freq.dtype == np.float64
    rows = (seq / "formants.csv").read_text().strip().splitlines()
    assert rows[0] == "frame,sections,status,found,F1,F2,F3,F4" and [r.split(",")[0] for r in rows[1:]] == ["0001", "0002", "0003"]
    sections = [int(r.split(",")[1]) for r in rows[1:]]
    assert len(set(sections)) > 1 and min(sections) >= 2          # the frames go through counts
    report = json.loads((seq / "formants.json").read_text())
    assert report["parameters"]["n_formants"] == 4 and report["parameters"]["to_cm"] == 136 * 1.6176470518112 / 10
    assert report["frames"] == 3 and sum(report["found"].values()) == 3
    assert report["status"]["ok"] + report["status"]["closed"] + report["status"]["non_finite"] >= 3
    status = np.array([int(r.split(",")[2]) for r in rows[1:]])
    found = np.array([int(r.split(",")[3]) for r in rows[1:]])
    assert (status & R.STATUS_NON_FINITE == 0).all() and (found >= 1).all()
    have = np.arange(4)[None, :] < found[:, None]
    assert np.isfinite(freq[have]).all() and np.isnan(freq[~have]).all() and (np.diff(freq, axis=1)[have[:, 1:]] > 0).all()
