"""The t-SNE kernels (artspeech_amd/csrc/tsne.hip) and the feature map built on them, stage by stage against the float64
restatement of tests/tsne_fp64.py, and end to end against scikit-learn's recorded runs on the fixture (tests/golden/tsne.npz;
neither scikit-learn nor the reference is imported here).  Every case is a few hundred points at most."""
import json
import os

import numpy as np
import pytest
import torch

import tsne_fp64 as R
from conftest import assert_grad_close, load_golden

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
# Worst relative difference of P (element by element, off the diagonal) and of beta between the device and the restatement over
# the cases of test_joint_probabilities, measured on an MI355X: 5.934e-08 (P, at N = 257; beta and the step counts were equal bit
# for bit in every case), recorded in profiles/tsne_parity.json.  The tolerance is 8 times that: the margin is for other shapes and compilers, the kernel itself is
# deterministic.
JOINT_P_WORST = 5.934e-08
JOINT_P_TOL = 8 * JOINT_P_WORST


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixture():
    g = load_golden("tsne")
    for a in g.values():
        a.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def fixture_P(fixture):
    """float32(scikit-learn's recorded P): the matrix the step tests give the device, and its float64 copy for the restatement."""
    P32 = fixture["P_sklearn"].astype(np.float32)
    P64 = P32.astype(np.float64)
    P64.setflags(write=False)
    return P32, P64


def _points(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    if N >= 4:
        X[N - 1] = X[0]                                              # two identical rows
        X[2] = X[1]
        X[2, D - 1] = np.nextafter(X[1, D - 1], np.float32(np.inf))   # two rows that differ in the last bit of one coordinate
    return X


# 63 / 64 / 65 and 127 / 128 / 129 straddle the 64-point tile, the D list its 32-column chunk (31, 32, 33) and the issue's widths
@pytest.mark.parametrize("N", [2, 63, 64, 65, 127, 128, 129, 200, 513])
def test_squared_distances(dev, N):
    from artspeech_amd.phoneme_recognition.tsne import squared_distances
    for D in (1, 3, 31, 32, 33, 128, 130):
        X = _points(N, D, 100 * N + D)
        wide = torch.full((N, D + 5), float("nan"), device=dev)     # a row stride larger than D; the padding is never read
        wide[:, :D] = torch.tensor(X, device=dev)
        got = squared_distances(wide[:, :D]).cpu().numpy()
        assert np.array_equal(squared_distances(torch.tensor(X, device=dev)).cpu().numpy(), got)
        ref = R.sqdist(X)
        assert (np.diag(got) == 0).all() and np.array_equal(got, got.T), (N, D)
        err = np.abs(got - ref)
        bound = (D + 4) * U24 * ref
        worst = float((err[ref > 0] / ref[ref > 0]).max()) / ((D + 4) * U24)
        print(f"sqdist N={N} D={D}: worst error {worst:.3f} of the bound")
        assert (err <= bound).all(), (N, D, worst)
        if N >= 4:
            assert got[0, N - 1] == 0.0 and got[1, 2] == np.float32(X[2, D - 1] - X[1, D - 1]) ** 2 > 0.0


def _joint_p_case(dev, X, perplexity):
    """(device outputs, restatement on the device's own float32 distances, worst relative difference of P and of beta)"""
    from artspeech_amd.phoneme_recognition import tsne
    dist = tsne.squared_distances(torch.tensor(X, device=dev))
    P, beta, H, steps = (t.cpu().numpy() for t in tsne.joint_probabilities(dist, perplexity))
    ref_P, ref_beta, ref_H, ref_steps = R.joint_probabilities(dist.cpu().numpy(), perplexity)
    N = len(X)
    assert P.dtype == np.float32 and beta.dtype == np.float64 and H.dtype == np.float64 and steps.dtype == np.int32
    assert ((np.abs(H - np.log(perplexity)) <= 1e-5) | (steps == 100)).all()
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    assert abs(P.astype(np.float64).sum() - 1.0) <= 2 * U24 + N * N * R.EPS
    assert np.array_equal(steps, ref_steps)
    off = ~np.eye(N, dtype=bool)
    worst_P = float((np.abs(P.astype(np.float64) - ref_P)[off] / ref_P[off]).max())
    worst_beta = float((np.abs(beta - ref_beta) / ref_beta).max())
    return (P, beta, H, steps), (ref_P, ref_beta), worst_P, worst_beta


JOINT_P_CASES = {"fixture": None, "N5": (5, 8, 2.0), "N65": (65, 8, 10.0), "N257": (257, 16, 30.0)}


@pytest.mark.parametrize("case", list(JOINT_P_CASES))
def test_joint_probabilities(dev, fixture, case):
    """Measured worst relative difference over these cases: 5.934e-08 for P (fixture 5.867e-08, N = 5 3.565e-08, N = 65
    5.808e-08, N = 257 5.934e-08: float32's half-ulp, 5.96e-08, the rounding of the stored P), 0 for beta, which like the step
    counts came out bit-equal; the tolerance of both is 8 times the worse of the two (JOINT_P_TOL = 4.75e-07).  On the fixture P is also compared with scikit-learn's recorded one, whose distances are scikit-learn's
    Gram-form ones: those differ from the direct differences by float32 roundings of d, which beta ~ 0.1 .. 1 turns into about
    1e-6 relative in P, so that comparison is relative to the largest entry."""
    if JOINT_P_CASES[case] is None:
        X, perplexity = fixture["X"], 10.0
    else:
        N, D, perplexity = JOINT_P_CASES[case]
        X = np.random.default_rng(N).standard_normal((N, D)).astype(np.float32)
    (P, beta, H, steps), (ref_P, ref_beta), worst_P, worst_beta = _joint_p_case(dev, X, perplexity)
    print(f"joint_p {case}: worst relative difference P {worst_P:.3e} beta {worst_beta:.3e}; steps {steps.min()}..{steps.max()}")
    assert worst_P <= JOINT_P_TOL and worst_beta <= JOINT_P_TOL, (worst_P, worst_beta)
    if case == "fixture":
        assert np.abs(P - fixture["P_sklearn"]).max() <= 1e-5 * fixture["P_sklearn"].max()


def test_identical_points_give_the_uniform_p(dev):
    X = np.full((20, 4), 0.75, np.float32)
    (P, beta, H, steps), _, worst_P, _ = _joint_p_case(dev, X, 5.0)
    off = ~np.eye(20, dtype=bool)
    assert (steps == 100).all() and (beta == 2.0 ** 99).all()
    assert (P[off] == P[0, 1]).all() and abs(float(P[0, 1]) * 20 * 19 - 1.0) <= U24 and worst_P <= U24


def _device_step(dev, P32, Y, update, gains, exaggeration, momentum, lr, n_iters=1):
    from artspeech_amd.phoneme_recognition import tsne
    t = [torch.tensor(np.asarray(a, dtype=np.float32), device=dev) for a in (P32, Y, update, gains)]
    grad = torch.empty_like(t[1])
    log = tsne.iterate(*t, n_iters, 0, exaggeration, momentum, lr, kl_every=1, grad=grad)
    return dict(Y=t[1].cpu().numpy(), update=t[2].cpu().numpy(), gains=t[3].cpu().numpy(), grad=grad.cpu().numpy(),
                log=log.cpu().numpy())


def _check_step(dev, what, P32, P64, Y, update, gains, exaggeration, momentum, lr):
    ref = R.descent_step(P64, Y.astype(np.float64), update.astype(np.float64), gains.astype(np.float64), exaggeration, momentum, lr)
    decided = np.abs(ref["decision"])
    assert decided[decided > 0].min() > 1e-4 * np.median(decided), what   # the inputs: no gain decision within rounding of zero
    got = _device_step(dev, P32, Y, update, gains, exaggeration, momentum, lr)
    for key in ("grad", "gains", "update", "Y"):
        assert_grad_close(got[key], ref[key], f"tsne {what} {key}")
    assert_grad_close(got["log"][0], [ref["grad_norm"], ref["gained_norm"], ref["kl"]], f"tsne {what} log")
    raised = got["gains"] > gains
    assert np.array_equal(raised[decided > 0], (ref["decision"] < 0)[decided > 0]), what   # +0.2 or x0.8: the same choice everywhere


@pytest.mark.parametrize("it,exaggeration,momentum", [(100, 12.0, 0.5), (280, 1.0, 0.8)])
def test_one_step_from_the_recorded_states(dev, fixture, fixture_P, it, exaggeration, momentum):
    P32, P64 = fixture_P
    _check_step(dev, f"iteration {it}", P32, P64, fixture[f"it{it}_Y"], fixture[f"it{it}_update"], fixture[f"it{it}_gains"],
                exaggeration, momentum, 50.0)


def _random_state(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.random((N, N)) ** 4
    P = A + A.T
    np.fill_diagonal(P, 0.0)
    P32 = (P / P.sum()).astype(np.float32)
    Y = (rng.standard_normal((N, 2)) * 3.0).astype(np.float32)
    update = (rng.standard_normal((N, 2)) * 0.1).astype(np.float32)
    gains = rng.uniform(0.01, 3.0, (N, 2)).astype(np.float32)
    gains[0] = 0.01   # at the floor: x0.8 is clipped back to it
    return P32, P32.astype(np.float64), Y, update, gains


# 2: one pair (at exaggeration 1 its two forces cancel exactly and there is no gradient to compare: 12 only); 16 / 17: one slab
# of 16 rows, then two; 65, 513: more slabs and tiles; 255 / 256 / 257: one tile of 256 points, then two
@pytest.mark.parametrize("N,exaggeration", [(2, 12.0)] + [(N, e) for N in (16, 17, 65, 255, 256, 257, 513) for e in (12.0, 1.0)])
def test_one_step_from_random_states(dev, N, exaggeration):
    """The state is drawn until the restatement finds no gain decision within 1e-4 of the median one (the margin the recorded
    states have; about one draw in ten has such a decision among its 2 N): a property of the inputs, found on the host."""
    momentum = 0.8 if exaggeration == 1.0 else 0.5
    for attempt in range(16):
        P32, P64, Y, update, gains = _random_state(N, N + 1000 * attempt)
        decided = np.abs(R.descent_step(P64, Y.astype(np.float64), update.astype(np.float64), gains.astype(np.float64), exaggeration,
                                        momentum, 200.0)["decision"])
        if decided[decided > 0].min() > 1e-4 * np.median(decided):
            break
    _check_step(dev, f"N={N} e={exaggeration:g}", P32, P64, Y, update, gains, exaggeration, momentum, 200.0)


def test_five_steps_from_the_pca_initialisation(dev, fixture, fixture_P):
    """Five and no more: float32 and float64 trajectories part at 3.8e-7 of max|Y| after 5 iterations, 1.6e-5 after 10 and 4e-2
    after 20 (the map is chaotic while P is exaggerated), so a longer comparison would test nothing."""
    P32, P64 = fixture_P
    Y0 = fixture["Y0"]
    Y, update, gains = Y0.astype(np.float64), np.zeros((len(Y0), 2)), np.ones((len(Y0), 2))
    for _ in range(5):
        s = R.descent_step(P64, Y, update, gains, 12.0, 0.5, 50.0)
        Y, update, gains = s["Y"], s["update"], s["gains"]
    got = _device_step(dev, P32, Y0, np.zeros_like(Y0), np.ones_like(Y0), 12.0, 0.5, 50.0, n_iters=5)
    assert_grad_close(got["Y"], Y, "tsne five steps Y")
    assert_grad_close(got["update"], update, "tsne five steps update")
    assert_grad_close(got["gains"], gains, "tsne five steps gains")
    assert_grad_close(got["log"][4], [s["grad_norm"], s["gained_norm"], s["kl"]], "tsne five steps log")
    assert np.isfinite(got["log"]).all() and got["log"].shape == (5, 3)


def test_pca_initialisation_is_the_restatements(dev, fixture):
    from artspeech_amd.phoneme_recognition.tsne import pca_init
    got = pca_init(torch.tensor(fixture["X"], device=dev)).cpu().numpy()
    assert got.dtype == np.float32 and np.abs(got - fixture["Y0"]).max() <= 4 * U24 * np.abs(fixture["Y0"]).max()
    assert abs(float(got[:, 0].std()) - 1e-4) <= 1e-10


def test_two_runs_with_one_seed_are_bit_equal(dev, fixture):
    from artspeech_amd.phoneme_recognition.tsne import TSNE
    X = torch.tensor(fixture["X"], device=dev)
    runs = []
    for _ in range(2):
        t = TSNE(perplexity=10.0, max_iter=300, init="random", random_state=0)
        runs.append((t.fit_transform(X).cpu().numpy(), t.log_, t.P_.cpu().numpy(), t.n_iter_))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    assert runs[0][2].tobytes() == runs[1][2].tobytes() and runs[0][3] == runs[1][3] == 299
    assert runs[0][1].shape == (300, 3) and np.isfinite(runs[0][1][49::50, 2]).all() and np.isnan(runs[0][1][0, 2])
    other = TSNE(perplexity=10.0, max_iter=300, init="random", random_state=1).fit_transform(X).cpu().numpy()
    assert other.tobytes() != runs[0][0].tobytes()


def test_end_to_end_on_the_fixture_is_within_scikit_learns_own_spread(dev, fixture):
    """No further from scikit-learn's worst run than scikit-learn's runs are from each other: KL <= max + (max - min) and
    trustworthiness (k = 5) >= min - (max - min) of its seven recorded runs."""
    from artspeech_amd.phoneme_recognition.tsne import TSNE
    t = TSNE(perplexity=10.0, max_iter=500, init="pca", random_state=0)
    Y = t.fit_transform(fixture["X"].copy())     # a host array is uploaded
    assert Y.is_cuda and Y.dtype == torch.float32 and tuple(Y.shape) == (200, 2) and Y is t.embedding_
    kl, trust = fixture["sk_kl"], fixture["sk_trust"]
    got_trust = R.trustworthiness(fixture["X"], Y.cpu().numpy(), 5)
    print(f"device KL {t.kl_divergence_:.4f} (scikit-learn {kl.min():.4f} .. {kl.max():.4f}), trustworthiness {got_trust:.4f} "
          f"(scikit-learn {trust.min():.4f} .. {trust.max():.4f}), n_iter_ {t.n_iter_}")
    assert t.kl_divergence_ <= kl.max() + (kl.max() - kl.min())
    assert got_trust >= trust.min() - (trust.max() - trust.min())
    assert t.n_iter_ == 499 and t.learning_rate_ == 50.0 and tuple(t.P_.shape) == (200, 200) and t.beta_.dtype == torch.float64
    assert t.kl_divergence_ == t.log_[-1, 2]


def test_run_test_writes_the_feature_map_and_nothing_else_changes(dev, tmp_path):
    from functools import partial

    from torch.utils.data import DataLoader

    from artspeech_amd.phoneme_recognition import (BLANK, PHONETIC_CLASSES, SIL, UNKNOWN, DeepSpeech2, Feature, Target, run_test)
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance
    phonetic = [t for tokens in PHONETIC_CLASSES.values() for t in tokens]
    vocabulary = {t: i for i, t in enumerate([BLANK, UNKNOWN, *phonetic, "x1", "x2"])}
    dataset = SyntheticPhonemeRecognitionDataset(8, vocabulary, n_articulators=2, n_samples=6, min_len=30, max_len=60, seed=2)
    loader = DataLoader(dataset, batch_size=4, shuffle=False, collate_fn=partial(collate_fn, features_names=[Feature.VOCAL_TRACT]))
    torch.manual_seed(0)
    model = DeepSpeech2(num_classes=len(vocabulary), in_channels=2, num_residual_layers=2, num_rnn_layers=2, rnn_hidden_size=16,
                        num_features=12, adapter_out_features=10, dropout=0.1).to(dev)
    decoder = GreedyCTCDecoder(tokens=list(vocabulary), sil_token=SIL, blank_token=BLANK, unk_word=UNKNOWN)
    call = dict(model=model, dataloader=loader, fn_metrics={"edit_distance": EditDistance(decoder)}, target=Target.CTC,
                feature=Feature.VOCAL_TRACT, device=dev, decoder=decoder, plot_target=Target.ARTICULATORY)
    plain = run_test(**call, save_dir=str(tmp_path / "plain"))
    assert sorted(os.listdir(tmp_path / "plain")) == ["confusion_matrix.npy", "substitution_matrix.npy"]
    options = dict(max_items_per_class=6, perplexity=8.0, max_iter=250, seed=3)
    told = run_test(**call, save_dir=str(tmp_path / "told"), model_features=options)
    assert told == plain and options == dict(max_items_per_class=6, perplexity=8.0, max_iter=250, seed=3)
    for name in ("confusion_matrix.npy", "substitution_matrix.npy"):
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "told" / name, "rb").read()
    written = set(os.listdir(tmp_path / "told")) - {"confusion_matrix.npy", "substitution_matrix.npy"}
    assert {"model_features_tsne.npy", "model_features_tokens.npy", "model_features_groups.npy", "model_features.json"} <= written
    assert written <= {"model_features_tsne.npy", "model_features_tokens.npy", "model_features_groups.npy", "model_features.json",
                       "model_features.pdf", "model_features_legend.pdf"}
    emb = np.load(tmp_path / "told" / "model_features_tsne.npy")
    tokens = np.load(tmp_path / "told" / "model_features_tokens.npy")
    groups = np.load(tmp_path / "told" / "model_features_groups.npy")
    M = len(tokens)
    assert emb.shape == (M, 2) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert tokens.dtype == np.int64 and groups.dtype == np.int64 and groups.shape == (M,) and M > 8
    names = {i: t for t, i in vocabulary.items()}
    group_of = {t: g for g, tokens_ in enumerate(PHONETIC_CLASSES.values()) for t in tokens_}
    assert all(names[int(t)] in group_of for t in tokens) and [group_of[names[int(t)]] for t in tokens] == groups.tolist()
    assert max(np.bincount(tokens)) <= 6
    with open(tmp_path / "told" / "model_features.json") as f:
        info = json.load(f)
    assert info["points"] == M == sum(info["points_per_group"].values()) and list(info["points_per_group"]) == [str(k) for k in PHONETIC_CLASSES]
    assert [info["points_per_group"][str(k)] for k in PHONETIC_CLASSES] == np.bincount(groups, minlength=len(PHONETIC_CLASSES)).tolist()
    assert info["perplexity"] == 8.0 and info["seed"] == 3 and info["n_iter"] == 249 and np.isfinite(info["kl_divergence"])
    assert info["learning_rate"] == 50.0


def test_refused_calls_name_their_entry_point_and_launch_nothing(dev):
    from artspeech_amd import _lib
    N = 8
    f = lambda *shape: torch.zeros(*shape, device=dev)   # noqa: E731
    P, Y, update, gains = f(N, N), f(N, 2), f(N, 2), torch.ones(N, 2, device=dev)
    log = torch.full((1, 3), 7.0, device=dev, dtype=torch.float64)
    need = _lib.call("as_tsne_workspace_bytes", N)
    ws = torch.zeros(need, device=dev, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="as_tsne_iterate.*at most 16384"):
        _lib.call("as_tsne_iterate", P, Y, update, gains, 16385, 1, 0, 50, 0, 1.0, 0.5, 50.0, 0.01, None, log, ws, need)
    with pytest.raises(RuntimeError, match=f"as_tsne_iterate.*workspace of {need - 16} bytes, {need} needed"):
        _lib.call("as_tsne_iterate", P, Y, update, gains, N, 1, 0, 50, 0, 1.0, 0.5, 50.0, 0.01, None, log, ws, need - 16)
    with pytest.raises(RuntimeError, match="as_tsne_joint_p.*workspace"):
        _lib.call("as_tsne_joint_p", P, N, 3.0, P, f(N).double(), f(N).double(), f(N).int(), ws, need - 16)
    with pytest.raises(RuntimeError, match="as_tsne_sqdist.*at most 16384"):
        _lib.call("as_tsne_sqdist", P, N, 16385, N, P)
    torch.cuda.synchronize()
    assert (log == 7.0).all() and (Y == 0).all() and (gains == 1).all() and (P == 0).all()
