"""Host-side pieces of the t-SNE feature map (no GPU): the float64 restatement of tests/tsne_fp64.py against scikit-learn's own
routines, the stopping rule on hand-made logs, the argument checks of ``TSNE`` and of the as_tsne_* entry points that are made
before anything is launched, and the frame selection on CPU tensors."""
import inspect
import os

import numpy as np
import pytest
import torch
import yaml

import tsne_fp64 as R
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def fixture():
    return load_golden("tsne")


@pytest.fixture(scope="module")
def restated(fixture):
    """(dist, P, beta, H, steps) of the restatement on the fixture at perplexity 10: computed once, shared, never written to."""
    dist = R.sqdist(fixture["X"])
    out = (dist,) + R.joint_probabilities(dist, 10.0)
    for a in out:
        a.setflags(write=False)
    return out


def _sklearn_private(*names):
    _t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    for name in names:
        if not hasattr(_t_sne, name):
            pytest.skip(f"sklearn.manifold._t_sne.{name} is not there")
    return _t_sne


def test_joint_probabilities_are_scikit_learns(fixture, restated):
    """P against _joint_probabilities and against the fixture's record of it.  scikit-learn returns neither beta nor the step
    count, so beta is read back from its conditional probabilities (log(c_ij / c_ik) = -beta (d_ij - d_ik)); the bisection only
    ever doubles, halves or takes a midpoint, so a beta equal to 1e-9 relative is the same path of the same number of steps."""
    _t_sne = _sklearn_private("_joint_probabilities", "_utils")
    from scipy.spatial.distance import squareform
    dist, P, beta, H, steps = restated
    d32 = dist.astype(np.float32)
    want = squareform(_t_sne._joint_probabilities(d32, 10.0, 0))
    assert np.abs(P - want).max() <= 1e-12 * want.max()
    assert np.abs(P - fixture["P_sklearn"]).max() <= 1e-5 * want.max()   # the record's distances are scikit-learn's Gram form
    C = _t_sne._utils._binary_search_perplexity(d32, 10.0, 0)
    for i in range(len(C)):
        j, k = np.argsort(d32[i])[[1, 6]]   # the nearest other point and the sixth: both probabilities far above underflow
        sk_beta = -np.log(C[i, j] / C[i, k]) / (float(d32[i, j]) - float(d32[i, k]))
        assert abs(sk_beta - beta[i]) <= 1e-9 * beta[i], i
    assert (np.abs(H - np.log(10.0)) <= 1e-5).all() and steps.max() < 100 and steps.min() >= 1
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all() and abs(P.sum() - 1.0) < P.size * R.EPS + 1e-13   # the clamp lifts the far pairs to eps


def test_bisection_cap_and_identical_points():
    """Identical points: every distance is 0, H = log(N - 1) whatever beta is, so the search runs its 100 steps (beta doubling all
    the way) and P is uniform."""
    dist = np.zeros((6, 6))
    P, beta, H, steps = R.joint_probabilities(dist, 2.0)
    assert (steps == 100).all() and (beta == 2.0 ** 99).all() and np.allclose(H, np.log(5.0))
    off = ~np.eye(6, dtype=bool)
    assert np.allclose(P[off], 1.0 / 30.0, rtol=1e-15) and (np.diag(P) == 0).all()


def test_kl_and_gradient_are_scikit_learns(fixture, restated):
    _t_sne = _sklearn_private("_kl_divergence")
    from scipy.spatial.distance import squareform
    P = restated[1]
    for it, e in ((100, 12.0), (280, 1.0)):
        Y = fixture[f"it{it}_Y"].astype(np.float64)
        kl, grad, _ = R.kl_and_gradient(P, Y, e)
        sk_kl, sk_grad = _t_sne._kl_divergence(Y.ravel(), squareform(P) * e, 1, len(Y), 2)
        assert np.abs(grad.ravel() - sk_grad).max() <= 1e-7 * np.abs(sk_grad).max()   # 4e-8 measured: the order of the sums
        if e == 1.0:   # scikit-learn's value is that of the P it is given; the restatement's is of the unexaggerated one
            assert abs(kl - sk_kl) <= 1e-12 * abs(sk_kl)


def test_five_descent_steps_are_scikit_learns(fixture, restated):
    _t_sne = _sklearn_private("_gradient_descent", "_kl_divergence")
    from scipy.spatial.distance import squareform
    P, Y0 = restated[1], fixture["Y0"].astype(np.float64)
    lr = R.auto_learning_rate(len(Y0))
    assert lr == 50.0
    p, error, it = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=5, n_iter_check=50,
                                            n_iter_without_progress=300, momentum=0.5, learning_rate=lr, min_gain=0.01,
                                            min_grad_norm=1e-7, verbose=0, args=[squareform(P) * 12.0, 1, len(Y0), 2], kwargs={})
    Y, _ = R.descend(P, Y0, 5)
    assert it == 4 and np.abs(Y.ravel() - p).max() <= 1e-9 * np.abs(p).max()


def test_trustworthiness_is_scikit_learns(fixture):
    manifold = pytest.importorskip("sklearn.manifold")
    X = fixture["X"]
    rng = np.random.default_rng(0)
    for Y in (fixture["it280_Y"], rng.standard_normal((len(X), 2))):
        for k in (5, 12):
            assert abs(R.trustworthiness(X, Y, k) - manifold.trustworthiness(X, Y, n_neighbors=k)) <= 1e-12


def _log(n, kl=None, gained=1.0):
    log = np.full((n, 3), np.nan)
    log[:, 0] = log[:, 1] = gained
    for i, v in (kl or {}).items():
        if i < n:
            log[i, 2] = v
    return log


@pytest.mark.parametrize("rule", ["package", "restatement"])
def test_stop_rule_on_hand_made_logs(rule):
    from artspeech_amd.phoneme_recognition import tsne
    stop = tsne.stop_rule if rule == "package" else R.stop_rule
    inf = float("inf")
    # progress at every check: never stops, the best follows
    log = _log(200, {49: 3.0, 99: 2.0, 149: 1.5, 199: 1.0})
    assert stop(log, 250, inf, 250, 300, 1e-7) == (None, 1.0, 449)
    # no new best for more than 300 iterations: best at 299, checks at 349 .. 599 (300 later: not yet), stops at 649
    kl = {i: 2.0 for i in range(49, 450, 50)}
    kl[49] = 1.0
    assert stop(_log(450, kl), 250, inf, 250, 300, 1e-7) == (649, 1.0, 299)
    assert stop(_log(350, kl), 250, inf, 250, 300, 1e-7) == (None, 1.0, 299)         # 599 - 299 = 300 is not more than 300
    # carried across chunks: the same answer from 50-iteration pieces
    best, best_iter, stopped = inf, 250, None
    for c in range(8):
        stopped, best, best_iter = stop(_log(450, kl)[50 * c: 50 * c + 50], 250 + 50 * c, best, best_iter, 300, 1e-7)
        assert (stopped is None) == (c < 7)
    assert (stopped, best, best_iter) == (649, 1.0, 299)
    # the gradient norm (of the gained gradient, column 1) at or below its threshold stops at that check, even on a new best
    log = _log(100, {49: 2.0, 99: 1.0})
    log[99, 1] = 1e-7
    log[98, 1] = 0.0   # not an iteration that is checked
    assert stop(log, 0, inf, 0, 300, 1e-7) == (99, 1.0, 99)
    log[:, 0] = 0.0    # the raw norm is not what is tested
    log[99, 1] = 2e-7
    assert stop(log, 0, inf, 0, 300, 1e-7) == (None, 1.0, 99)
    # the exploration phase: patience 250 over 250 iterations can never run out (249 - 49 = 200)
    assert stop(_log(250, {49: 1.0, 99: 2.0, 149: 2.0, 199: 2.0, 249: 2.0}), 0, inf, 0, 250, 1e-7) == (None, 1.0, 49)
    # a NaN divergence is no progress
    assert stop(_log(50, {49: float("nan")}), 0, inf, 0, 300, 1e-7) == (None, inf, 0)


def test_tsne_checks_its_arguments_before_it_needs_a_device():
    from artspeech_amd.phoneme_recognition.tsne import TSNE
    X = torch.randn(20, 4)
    sig = inspect.signature(TSNE.__init__)
    assert list(sig.parameters)[1:] == ["n_components", "perplexity", "early_exaggeration", "learning_rate", "max_iter",
                                        "n_iter_without_progress", "min_grad_norm", "metric", "init", "random_state", "method"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in sig.parameters.items() if name not in ("self", "n_components"))
    assert (sig.parameters["method"].default, sig.parameters["perplexity"].default, sig.parameters["init"].default) == ("exact", 30.0, "pca")
    with pytest.raises(ValueError, match="perplexity"):
        TSNE(perplexity=20.0).fit(X)
    with pytest.raises(ValueError, match="perplexity"):
        TSNE(perplexity=0.0).fit(X)
    with pytest.raises(ValueError, match="n_components"):
        TSNE(n_components=3, perplexity=5.0).fit(X)
    with pytest.raises(NotImplementedError, match="barnes_hut"):
        TSNE(perplexity=5.0, method="barnes_hut").fit_transform(X)
    with pytest.raises(ValueError, match="metric"):
        TSNE(perplexity=5.0, metric="cosine").fit(X)
    for bad in (float("nan"), float("inf")):
        Xb = X.clone()
        Xb[3, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            TSNE(perplexity=5.0).fit(Xb)
    with pytest.raises(ValueError, match="init"):
        TSNE(perplexity=5.0, init=np.zeros((19, 2))).fit(X)
    with pytest.raises(ValueError, match="max_iter"):
        TSNE(perplexity=5.0, max_iter=100).fit(X)


def test_symbols_are_declared_bound_and_exported():
    from artspeech_amd import _lib, build
    L = _lib.lib()
    names = ("as_tsne_sqdist", "as_tsne_joint_p", "as_tsne_iterate", "as_tsne_workspace_bytes")
    for name in names:
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    assert all(_lib.PROTOTYPES[n][1][-1] is _lib.Stream for n in names[:3]) and _lib.PROTOTYPES[names[3]][0] is _lib.C.c_int64
    assert build.SOURCES["tsne.hip"] == [] and os.path.exists(os.path.join(build.CSRC, "tsne.hip"))
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    for cite in ("phoneme_recognition/__init__.py:355-356", "_joint_probabilities", "_binary_search_perplexity", "_kl_divergence",
                 "_gradient_descent"):
        assert cite in header, cite


def test_workspace_size_follows_the_plan():
    from artspeech_amd import _lib
    ws = [_lib.call("as_tsne_workspace_bytes", n) for n in (2, 256, 257, 3300, 8192, 16384)]
    assert all(b > 0 and b % 16 == 0 for b in ws) and ws == sorted(ws)
    assert ws[3] < 8 << 20   # the thesis size: 64 slabs x 4 x 3300 floats and change
    assert [_lib.call("as_tsne_workspace_bytes", n) for n in (-1, 0, 1, 16385)] == [0, 0, 0, 0]


def test_bad_arguments_are_refused_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail otherwise (or crash); these return the library's message."""
    from artspeech_amd import _lib
    big = 1 << 30
    for args in ((None, 4, 8, 4, 16), (16, 4, 8, 4, None), (16, 4, 1, 4, 16), (16, 4, 16385, 4, 16), (16, 4, 8, 0, 16),
                 (16, 3, 8, 4, 16)):
        with pytest.raises(RuntimeError, match=r"^as_tsne_sqdist failed \(code -1\): as_tsne_sqdist: "):
            _lib.call("as_tsne_sqdist", *args, stream=0)
    ok = dict(dist=16, N=8, perplexity=3.0, P=16, beta=16, entropy=16, steps=16, ws=16, ws_bytes=big)
    for change in (dict(dist=None), dict(P=None), dict(beta=None), dict(entropy=None), dict(steps=None), dict(N=1), dict(N=16385),
                   dict(perplexity=0.0), dict(perplexity=-1.0), dict(perplexity=8.0), dict(perplexity=float("nan"))):
        with pytest.raises(RuntimeError, match=r"^as_tsne_joint_p failed \(code -1\): as_tsne_joint_p: "):
            _lib.call("as_tsne_joint_p", *dict(ok, **change).values(), stream=0)
    need = _lib.call("as_tsne_workspace_bytes", 8)
    for change in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=24)):
        with pytest.raises(RuntimeError, match=rf"^as_tsne_joint_p failed \(code -3\): as_tsne_joint_p: workspace.*{need} needed"):
            _lib.call("as_tsne_joint_p", *dict(ok, **change).values(), stream=0)
    ok = dict(P=16, Y=16, update=16, gains=16, N=8, n_iters=1, it0=0, kl_every=50, kl_last=0, e=12.0, m=0.5, lr=50.0, min_gain=0.01,
              grad=None, log=16, ws=16, ws_bytes=big)
    for change in (dict(P=None), dict(Y=None), dict(update=None), dict(gains=None), dict(log=None), dict(N=1), dict(N=16385),
                   dict(n_iters=0), dict(it0=-1), dict(kl_every=-1), dict(Y=20)):
        with pytest.raises(RuntimeError, match=r"^as_tsne_iterate failed \(code -1\): as_tsne_iterate: "):
            _lib.call("as_tsne_iterate", *dict(ok, **change).values(), stream=0)
    with pytest.raises(RuntimeError, match=r"^as_tsne_iterate failed \(code -3\): as_tsne_iterate: workspace"):
        _lib.call("as_tsne_iterate", *dict(ok, ws_bytes=need - 1).values(), stream=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.call("as_tsne_sqdist", torch.zeros(4, 4), 4, 4, 4, 16, stream=0)


def test_sample_features_per_class_on_cpu_tensors():
    from artspeech_amd.phoneme_recognition.tsne import sample_features_per_class
    g = torch.Generator().manual_seed(3)
    targets = torch.randint(0, 9, (600,), generator=g)
    targets[targets == 7] = 8                                  # token 7 has no frame
    features = torch.arange(600, dtype=torch.float32)[:, None] * torch.ones(1, 3)   # a row names its frame
    few = int((targets == 2).sum())
    assert 20 < few < 100
    ids = [5, 2, 7, 0]

    def draw(seed, max_items=40):
        return sample_features_per_class(features, targets, ids, max_items, torch.Generator().manual_seed(seed))

    feats, tokens = draw(0)
    assert feats.shape == (len(tokens), 3) and tokens.dtype == targets.dtype
    frames = feats[:, 0].long()
    assert torch.equal(targets[frames], tokens)                                   # a feature row with its own target
    assert len(set(frames.tolist())) == len(frames)                               # no frame twice
    assert tokens.unique_consecutive().tolist() == [5, 2, 0]                      # only listed tokens, in the list's order
    assert all(int((tokens == t).sum()) == min(40, int((targets == t).sum())) for t in (5, 2, 0))
    again = draw(0)
    assert torch.equal(again[0], feats) and torch.equal(again[1], tokens)         # reproducible for a seed
    assert not torch.equal(draw(1)[0], feats)
    everything = draw(0, 1000)[1]
    assert int((everything == 2).sum()) == few                                    # fewer frames than asked: all of them, once
    empty = sample_features_per_class(features, targets, [7], 10)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)
    with pytest.raises(ValueError, match="max_items_per_class"):
        sample_features_per_class(features, targets, ids, 0)
    with pytest.raises(ValueError, match="features"):
        sample_features_per_class(features, targets[:-1], ids)


def test_features_config_is_the_synthetic_one_plus_its_block():
    import embed_phoneme_recognition as E
    import test_phoneme_recognition as plain
    from artspeech_amd.phoneme_recognition import run_test
    from train_phoneme_recognition import build_vocabulary
    from artspeech_amd.phoneme_recognition import Criterion
    with open(os.path.join(ROOT, "configs", "test_recognizer_features_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", "test_recognizer_synthetic.yaml")) as f:
        base = yaml.safe_load(f)
    assert set(cfg) <= set(inspect.signature(E.main).parameters)
    assert {k for k in cfg if cfg[k] != base.get(k)} == {"model_features", "save_dir"} and set(base) <= set(cfg)
    block = cfg["model_features"]
    assert block["max_items_per_class"] == 100 and block["perplexity"] == 30.0 and block["seed"] == 0
    vocabulary = build_vocabulary(None, Criterion.CTC)
    tokens = [t for group in block["groups"].values() for t in group]
    assert len(tokens) == len(set(tokens)) == 42 and set(tokens) <= set(vocabulary)
    params = inspect.signature(run_test).parameters
    assert params["model_features"].default is None and params["model_features"].kind is inspect.Parameter.KEYWORD_ONLY
    # test_phoneme_recognition.main's parameters, in its order and with its defaults, then `model_features`
    params = list(inspect.signature(E.main).parameters.values())
    assert params[:-1] == list(inspect.signature(plain.main).parameters.values())
    assert params[-1].name == "model_features" and params[-1].default is None
    with pytest.raises(NotImplementedError, match="CTC"):
        E.main(**dict(cfg, loss="CE"))
    with pytest.raises(ValueError, match="save_dir and a plot_target"):
        E.main(**dict(cfg, plot_target=None))
    with pytest.raises(ValueError, match="save_dir and a plot_target"):
        run_test(torch.nn.Identity(), [], {}, None, device="cpu", model_features={})
