"""Host-side pieces of the contour smoothing and of the synthesis entry point (no GPU): the restatement of
tests/contour_spline_fp64.py against scipy and against the properties its definition promises, the conditioning that the device
test's tolerance rests on, and the plumbing (symbol, configs, a script that imports cleanly)."""
import importlib
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import yaml

import contour_spline_fp64 as R
from conftest import ROOT


@pytest.mark.parametrize("d,K", [(1, 2), (1, 7), (2, 3), (2, 12), (3, 4), (3, 12), (3, 32)])
def test_restatement_is_scipys_design_matrix_and_a_dense_solve(d, K):
    scipy_interpolate = pytest.importorskip("scipy.interpolate")
    rng = np.random.default_rng(d * 100 + K)
    pts = R.smooth_curve(rng, 41).astype(np.float64)
    u = R.parameter(pts)
    knots = R.knot_vector(K, d)
    assert len(knots) == K + d + 1
    B = scipy_interpolate.BSpline.design_matrix(u, knots, d).toarray()
    assert np.abs(R.design_matrix(u, K, d) - B).max() <= 4e-16
    D = np.diff(np.eye(K), n=2, axis=0) if K > 2 else np.zeros((0, K))
    for lam in (1e-6, 1e-3, 1.0):
        c = np.linalg.solve(B.T @ B + lam * (D.T @ D), B.T @ pts)
        v = np.linspace(0.0, 1.0, 23)
        want = (scipy_interpolate.BSpline.design_matrix(v, knots, d).toarray() @ c).T
        got = R.smooth(pts, d, K, lam, 23)
        cond = np.linalg.cond(B.T @ B + lam * (D.T @ D))
        assert np.abs(got - want).max() <= 8 * cond * 2.0 ** -52, (lam, cond)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_collinear_evenly_spaced_points_are_reproduced_for_any_lambda(d):
    """What "reproduced" can mean under the definition.  The control points of the line u -> a + b u sit at the Greville abscissae
    of the knot vector.  For d = 1 those are evenly spaced: the line's control points have no second difference, the penalty does
    not see it, and the points come back one by one for any lambda.  For d = 2 and 3 the abscissae of a CLAMPED vector bunch at
    the ends, so the penalty does pull on a line's control points: the outputs stay ON the line for any lambda (both coordinates
    are the same affine function of one fitted scalar), they slide along it by an amount that goes to zero with lambda (3.3e-8,
    3.3e-5, 1.2e-2, 3.3e-2 of the unit square at lambda = 1e-6, 1e-3, 1, 1e6 for d = 3) and keep their order."""
    t = np.linspace(0.0, 1.0, 17)
    pts = np.stack([0.2 + 0.5 * t, 0.9 - 0.3 * t], axis=1)
    normal = np.array([0.3, 0.5]) / np.hypot(0.3, 0.5)
    for lam in (1e-6, 1e-3, 1.0, 1e6):
        got = R.smooth(pts, d, 9, lam).T
        assert np.abs((got - pts[0]) @ normal).max() <= 1e-8, lam       # on the line, for every degree and lambda
        along = (got - pts[0]) @ (pts[-1] - pts[0]) / ((pts[-1] - pts[0]) ** 2).sum()
        assert (np.diff(along) > 0).all(), lam                          # and in order along it
        if d == 1:
            assert np.abs(got - pts).max() <= 1e-8, lam
    assert np.abs(R.smooth(pts, d, 9, 1e-12).T - pts).max() <= 1e-9    # and point by point as lambda goes to zero


@pytest.mark.parametrize("d", [1, 2, 3])
def test_a_very_large_lambda_approaches_the_least_squares_line(d):
    """lambda -> infinity leaves only control points without second difference: evenly spaced on a line, c_j = a + b j / (K-1).
    The curve is then a + b g(u) with g the spline of the control values j / (K-1), and the fit is the least-squares regression of
    the points on (1, g(u)): a straight line.  For d = 1, g(u) = u, the ordinary least-squares line in the parameter."""
    rng = np.random.default_rng(3)
    pts = R.smooth_curve(rng, 40).astype(np.float64)
    u = R.parameter(pts)
    K = 12
    ramp = np.arange(K) / (K - 1.0)
    g = R.design_matrix(u, K, d) @ ramp
    coef, *_ = np.linalg.lstsq(np.stack([np.ones_like(g), g], axis=1), pts, rcond=None)
    v = np.arange(40) / 39.0
    gv = R.design_matrix(v, K, d) @ ramp
    want = (coef[0][:, None] + coef[1][:, None] * gv)
    assert np.abs(R.smooth(pts, d, K, 1e9) - want).max() <= 1e-6
    if d == 1:
        line = np.polyfit(u, pts, 1)
        assert np.abs(want - (line[0][:, None] * v + line[1][:, None])).max() <= 1e-12
    assert np.abs(R.smooth(pts, d, K, 1e-3) - want).max() > 1e-3   # and an ordinary lambda does follow the curve


def test_fit_is_invariant_to_translation():
    rng = np.random.default_rng(4)
    pts = R.clustered_contour(rng, 33).astype(np.float64)
    shift = np.array([3.25, -1.5])
    assert np.abs(R.smooth(pts + shift, 3, 12, 1e-3) - (R.smooth(pts, 3, 12, 1e-3) + shift[:, None])).max() <= 1e-10


def test_repeated_points_two_points_and_zero_length():
    rng = np.random.default_rng(5)
    rep = R.repeated_contour(rng, 30).astype(np.float64)
    assert (np.diff(rep, axis=0) == 0).all(axis=1).any()          # it does hold repeated points
    out = R.smooth(rep, 3, 12, 1e-3)
    assert np.isfinite(out).all() and np.abs(out[:, 0] - rep[0]).max() < 0.05 and np.abs(out[:, -1] - rep[-1]).max() < 0.05
    two = np.array([[0.1, 0.2], [0.7, 0.4]])
    got = R.smooth(two, 3, 4, 1e-3, 5)
    want = two[0][:, None] + (two[1] - two[0])[:, None] * (np.arange(5) / 4.0)   # the chord: two points are collinear
    assert np.abs(got - want).max() <= 1e-9
    still = np.repeat(np.array([[0.3, 0.6]], dtype=np.float32), 6, axis=0)
    assert np.array_equal(R.smooth(still, 3, 12, 1e-3, 9), np.repeat(still[0].astype(np.float64)[:, None], 9, axis=1))
    assert np.isnan(R.smooth(np.array([[0.0, 0.0], [np.nan, 1.0]]), 1, 2, 1.0)).all()


def test_every_matrix_of_the_device_tests_is_conditioned_below_1e8():
    """The premise of the device test's tolerance: two float64 solves of one system differ by about cond * 2^-52 <= 2.2e-8 relative,
    under half of float32's half-ulp, so that at most a rounding flip of one float32 ulp is left."""
    worst = 0.0
    for n, N, K, d, M, lam in R.PARITY_CASES:
        K = d + 1 if K is None else K
        for c in R.case_contours(n, N):
            worst = max(worst, np.linalg.cond(R.normal_matrix(c.T, K, d, lam)))
    d, K, lam = R.DEFAULTS
    for N in (50, 64):
        for c in R.case_contours(24, N, seed=7):   # the layout, lengths and edge-case tests draw from these
            worst = max(worst, np.linalg.cond(R.normal_matrix(c.T, K, d, lam)))
    print(f"worst condition number {worst:.3e}")
    assert worst <= 1e8, worst


def test_symbol_is_declared_bound_and_exported():
    from artspeech_amd import _lib, build
    L = _lib.lib()
    assert "as_contour_spline" in _lib.PROTOTYPES and hasattr(L, "as_contour_spline")
    res, args = _lib.PROTOTYPES["as_contour_spline"]
    assert len(args) == 17 and args[-1] is _lib.Stream and args[8] is _lib.C.c_double
    assert build.SOURCES["contour_spline.hip"] == [] and os.path.exists(os.path.join(build.CSRC, "contour_spline.hip"))
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    for site in ("generate_vocal_tract_shape_v2.py:173,252", "generate_vocal_tract_shape.py:155", "__init__.py:178-180", "unpinned"):
        assert site in header, site


def test_limits_are_refused_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail otherwise (or crash); these return the library's message."""
    from artspeech_amd import _lib
    ok = dict(N=50, K=12, degree=3, lam=1e-3, M=50)
    bad = [dict(N=1), dict(N=257), dict(K=3), dict(K=33), dict(M=1), dict(M=1025), dict(degree=0), dict(degree=4), dict(lam=0.0),
           dict(lam=-1.0), dict(lam=float("inf")), dict(lam=float("nan"))]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(RuntimeError, match="as_contour_spline failed"):
            _lib.call("as_contour_spline", 16, 2 * a["N"], a["N"], 1, 4, a["N"], a["K"], a["degree"], a["lam"], a["M"], None, 0, 0, 16,
                      a["M"], None, stream=0)
    with pytest.raises(RuntimeError, match="as_contour_spline failed"):   # an output row shorter than M
        _lib.call("as_contour_spline", 16, 100, 50, 1, 4, 50, 12, 3, 1e-3, 50, None, 0, 0, 16, 49, None, stream=0)
    with pytest.raises(RuntimeError, match="B \\* T \\* A"):              # lengths with a count that is no multiple of T * A
        _lib.call("as_contour_spline", 16, 100, 50, 1, 7, 50, 12, 3, 1e-3, 50, 16, 2, 3, 16, 50, None, stream=0)


def test_cpu_tensors_raise_and_save_outputs_still_refuses():
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    with pytest.raises(RuntimeError, match="MI355X"):
        regularize_contours(torch.zeros(3, 2, 50))
    from artspeech_amd.phoneme_to_articulation import save_outputs
    with pytest.raises(NotImplementedError):   # unchanged: the regularised dumps come from generate_vocal_tract_shape.py
        save_outputs([], [], torch.zeros(0), torch.zeros(0), [], [], [], "unused", regularize_out=True)


CONFIGS = ("generate_vocal_tract_shape_synthetic.yaml", "generate_vocal_tract_shape_mean_contour_synthetic.yaml",
           "generate_vocal_tract_shape_aligned_synthetic.yaml")


@pytest.mark.parametrize("name", CONFIGS)
def test_configs_parse_into_mains_keywords(name):
    import inspect
    import generate_vocal_tract_shape as S
    params = set(inspect.signature(S.main).parameters)
    with open(os.path.join(ROOT, "configs", name)) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= params, set(cfg) - params
    assert cfg["method"] in S.METHODS and cfg["save_to"].startswith("results/")
    assert os.path.dirname(cfg["state_dict_filepath"]) in {os.path.dirname(p) for p in _written_by_training_configs()}
    if "alignments_dir" in cfg:
        with open(os.path.join(ROOT, "configs", "align_recognizer_synthetic.yaml")) as f:
            assert cfg["alignments_dir"] == os.path.join(yaml.safe_load(f)["save_dir"], "alignments")


def _written_by_training_configs():
    out = []
    for name in os.listdir(os.path.join(ROOT, "configs")):
        if name.startswith("train_") and name.endswith(".yaml"):
            with open(os.path.join(ROOT, "configs", name)) as f:
                results_dir = yaml.safe_load(f).get("results_dir")
            if results_dir:
                out.append(os.path.join(results_dir, "best_model.pt"))
    return out


def test_importing_the_script_creates_nothing(tmp_path, monkeypatch):
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delitem(sys.modules, "generate_vocal_tract_shape", raising=False)
    module = importlib.import_module("generate_vocal_tract_shape")
    assert callable(module.main) and os.path.dirname(module.__file__) == ROOT
    assert os.listdir(tmp_path) == []
    assert not module.__name__.startswith(("train_", "test_"))


def test_sentence_files_and_batches(tmp_path):
    """The host half of synthesize(): target_sequence.txt files read back, unknown tokens numerised as <unk>, sentences sorted by
    length (descending, as the models' packed recurrences want) and cut into batches that keep every sentence once."""
    from artspeech_amd.phoneme_to_articulation import synthesis as S
    vocabulary = {"<blank>": 0, "<unk>": 1, "a": 2, "b": 3}
    (tmp_path / "s1.txt").write_text("a a b")
    (tmp_path / "s2.txt").write_text("b zz a a a\n")
    al = tmp_path / "alignments"
    al.mkdir()
    (al / "3_phonemes.txt").write_text("a")
    (al / "10_phonemes.txt").write_text("b b")
    (al / "3.csv").write_text("ignored")
    (al / "4_phonemes.txt").write_text("")   # an utterance without alignment: no frames, left out
    sentences = S.read_sentences([{"name": "one", "phonemes_filepath": str(tmp_path / "s1.txt")},
                                  {"name": "two", "phonemes_filepath": str(tmp_path / "s2.txt")}], str(al))
    assert [(n, t) for n, t in sentences] == [("one", ["a", "a", "b"]), ("two", ["b", "zz", "a", "a", "a"]), ("3", ["a"]),
                                              ("10", ["b", "b"])]
    assert S.numerize(["b", "zz", "a"], vocabulary).tolist() == [3, 1, 2]
    batches = S.make_batches(sentences, 3)
    assert [[sentences[i][0] for i in b] for b in batches] == [["two", "one", "10"], ["3"]]
    with pytest.raises(ValueError, match="twice"):
        S.read_sentences([{"name": "3", "phonemes_filepath": str(tmp_path / "s1.txt")}], str(al))
    with pytest.raises(ValueError, match="no sentence"):
        S.read_sentences(None, None)
