"""as_ctc_align / forced_align on the device against the fp64 restatement (tests/forced_align_fp64.py).

Exact cases use log-probabilities that are multiples of 1/8 in [-16, 0]: every partial sum of at most 8192 of them is an integer
multiple of 1/8 below 2^24 / 8, so fp32 accumulates them exactly, the float32 and float64 recursions take the same decisions (ties
included, tests/test_forced_align_host.py) and every output must equal the oracle's bit for bit; span_score, a mean, to one fp32
rounding.  Rounded cases (log-softmax of 3 * randn) may differ from the fp64 optimum at a near-tie, so they check what must hold
regardless: a valid path, |score - rescore64(path)| <= bound and optimum64 - rescore64(path) <= 2 * bound with
bound = (Tb^2 + 4 Tb) * M * 2^-24, M the largest finite |log-probability| of the utterance's valid frames: the worst-case rounding
of Tb fp32 additions of partial sums up to Tb * M, plus the rounding of x - lse."""
import os

import numpy as np
import pytest
import torch

import forced_align_fp64 as F
from conftest import ROOT

pytestmark = pytest.mark.gpu

FRAME_KEYS = ("frame_index", "frame_token", "frame_filled")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def grid(rng, B, T, C):
    return (-rng.integers(0, 129, size=(B, T, C)) / 8.0).astype(np.float32)


def labels_without_repeats(rng, n, C, blank=0):
    """n labels, none equal to its neighbour (so n frames are enough)"""
    pool = [c for c in range(C) if c != blank]
    out = []
    for _ in range(n):
        out.append(int(rng.choice([c for c in pool if not out or c != out[-1]])))
    return out


def pad(targets, width=None):
    width = max([len(t) for t in targets] + [0]) if width is None else width
    out = np.full((len(targets), width), -1, dtype=np.int64)
    for b, t in enumerate(targets):
        out[b, : len(t)] = t
    return out


def to_host(al):
    return {k: getattr(al, k).cpu().numpy() for k in ("score", "feasible", *FRAME_KEYS, "spans", "span_score")}


def assert_same_outputs(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def run(dev, logp, targets, il, tl, blank=0, logits=False):
    from artspeech_amd.phoneme_recognition import forced_align
    al = forced_align(torch.from_numpy(logp).to(dev), torch.from_numpy(pad(targets)).to(dev), il, tl, blank, logits)
    torch.cuda.synchronize()
    return to_host(al)


def assert_exact(got, logp, targets, il, tl, blank):
    want = F.align_batch(logp.astype(np.float64), [np.asarray(t) for t in targets], il, tl, blank)
    assert got["score"].dtype == np.float32
    assert np.array_equal(got["score"], want["score"].astype(np.float32)), (got["score"], want["score"])
    assert np.array_equal(got["feasible"], np.isfinite(want["score"]))
    for k in (*FRAME_KEYS, "spans"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    nan = np.isnan(want["span_score"])
    assert np.array_equal(np.isnan(got["span_score"]), nan)
    mean = want["span_score"][~nan]
    assert (np.abs(got["span_score"][~nan].astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all()
    return want


def exact_case(dev, rng, T, C, targets, il, blank=0):
    tl = [len(t) for t in targets]
    logp = grid(rng, len(targets), T, C)
    got = run(dev, logp, targets, il, tl, blank)
    return got, assert_exact(got, logp, targets, il, tl, blank)


def test_all_blank(dev):
    got, _ = exact_case(dev, np.random.default_rng(1), 6, 4, [[], [], []], [5, 3, 1])
    assert (got["frame_filled"] == -1).all() and (got["frame_token"][0, :5] == 0).all() and got["spans"].shape == (3, 0, 2)


def test_one_label_one_frame(dev):
    got, _ = exact_case(dev, np.random.default_rng(2), 4, 5, [[3], [2], []], [1, 3, 1])
    assert got["frame_index"][0, 0] == 0 and got["spans"][0, 0].tolist() == [0, 1]


def test_as_many_frames_as_labels(dev):
    got, _ = exact_case(dev, np.random.default_rng(3), 5, 6, [[1, 2, 3, 4], [5, 1, 5], [2, 3]], [4, 3, 2])
    assert got["feasible"].all() and (got["frame_index"][0, :4] == np.arange(4)).all()


def test_adjacent_equal_labels_at_the_minimum_length_and_one_frame_short(dev):
    repeated = [1, 1, 2, 2, 2]   # 5 labels, 3 adjacent equal pairs: 8 frames at least
    got, _ = exact_case(dev, np.random.default_rng(4), 9, 4, [repeated, repeated, [3, 3]], [8, 7, 3])
    assert got["feasible"].tolist() == [True, False, True] and got["score"][1] == -np.inf
    assert (got["frame_index"][1] == -1).all() and (got["spans"][1] == -1).all() and np.isnan(got["span_score"][1]).all()
    assert got["frame_index"][0, :8].tolist() == [0, -1, 1, 2, -1, 3, -1, 4]


def test_no_frames(dev):
    got, _ = exact_case(dev, np.random.default_rng(5), 4, 4, [[], [1, 2], [3]], [0, 0, 4])
    assert got["score"][0] == 0.0 and got["score"][1] == -np.inf and got["feasible"].tolist() == [True, False, True]


def test_two_classes(dev):
    exact_case(dev, np.random.default_rng(6), 9, 2, [[1, 1, 1], [1], [1, 1]], [5, 9, 4])


def test_blank_is_not_class_zero(dev):
    rng = np.random.default_rng(7)
    got, _ = exact_case(dev, rng, 12, 5, [[0, 1, 0, 4], [3, 3], [4]], [12, 7, 2], blank=2)
    assert set(got["frame_token"][0].tolist()) <= {0, 1, 2, 4, -1}


@pytest.mark.parametrize("L", [127, 128])
def test_state_count_boundary_of_the_two_exchange_paths(dev, L):
    """S = 255 states fit the one-wave kernel (4 states per lane), S = 257 take the 256-thread kernel and its LDS exchange"""
    rng = np.random.default_rng(L)
    targets = [labels_without_repeats(rng, L, 6), labels_without_repeats(rng, 60, 6), labels_without_repeats(rng, L - 1, 6)]
    targets[1][10] = targets[1][9]   # one repeat
    got, _ = exact_case(dev, rng, 140, 6, targets, [140, 61, 133])
    assert got["feasible"].all()


def test_largest_table_in_the_workspace(dev):
    from artspeech_amd import _lib
    rng = np.random.default_rng(8)
    targets = [labels_without_repeats(rng, 2047, 6), labels_without_repeats(rng, 1000, 6), [1, 1, 2]]
    assert _lib.call("as_ctc_align_workspace_bytes", 2100, 3, 2047) == 3 * 2100 * 1024
    got, _ = exact_case(dev, rng, 2100, 6, targets, [2100, 2050, 2100])
    assert got["feasible"].all()


def test_workspace_and_lds_tables_give_the_same_paths(dev):
    """T = 1024, L = 512 (the table goes where the library chooses: the workspace), and a slice of the same inputs at T = 64,
    L = 16, where the size call returns 0 and the table lives in LDS"""
    from artspeech_amd import _lib
    rng = np.random.default_rng(9)
    targets = [labels_without_repeats(rng, 512, 7), labels_without_repeats(rng, 300, 7), labels_without_repeats(rng, 40, 7)]
    logp = grid(rng, 3, 1024, 7)
    il = [1024, 700, 41]
    got = run(dev, logp, targets, il, [512, 300, 40])
    assert_exact(got, logp, targets, il, [512, 300, 40], 0)
    assert _lib.call("as_ctc_align_workspace_bytes", 64, 3, 16) == 0
    small_t, small_il = [t[:n] for t, n in zip(targets, (16, 9, 12))], [64, 20, 33]
    small = run(dev, logp[:, :64].copy(), small_t, small_il, [16, 9, 12])
    assert_exact(small, logp[:, :64], small_t, small_il, [16, 9, 12], 0)


def _mixed_case(rng):
    targets = [[1, 2, 2, 3], [4], [], [3, 1, 3, 1, 2]]
    return grid(rng, 4, 14, 5), targets, [14, 6, 3, 9], [4, 1, 0, 5]


def test_permuted_view_and_concatenated_targets(dev):
    from artspeech_amd.phoneme_recognition import forced_align
    logp, targets, il, tl = _mixed_case(np.random.default_rng(10))
    want = run(dev, logp, targets, il, tl)
    assert_exact(want, logp, targets, il, tl, 0)
    tbc = torch.from_numpy(np.ascontiguousarray(logp.transpose(1, 0, 2))).to(dev)   # (T, B, C), as the loss takes it
    view = tbc.permute(1, 0, 2)
    assert not view.is_contiguous() and view.stride(2) == 1
    padded = torch.from_numpy(pad(targets, 7)).to(dev)
    assert_same_outputs(to_host(forced_align(view, padded, il, tl)), want)
    flat = torch.tensor([v for t in targets for v in t], dtype=torch.int64)
    assert_same_outputs(to_host(forced_align(view, flat, torch.tensor(il), torch.tensor(tl))), want)


def test_each_optional_output_may_be_null_and_limits_are_refused_before_any_launch(dev):
    from artspeech_amd import _lib
    logp, targets, il, tl = _mixed_case(np.random.default_rng(11))
    B, T, C = logp.shape
    max_l = max(tl)
    x, tg = torch.from_numpy(logp).to(dev), torch.from_numpy(pad(targets)).to(dev)
    il_d, tl_d = torch.tensor(il, device=dev), torch.tensor(tl, device=dev)
    names = (*FRAME_KEYS, "spans", "span_score")

    def call(null=None, T_arg=T, max_l_arg=max_l, ws=None, ws_bytes=0):
        out = {"score": torch.full((B,), 7.0, device=dev), "spans": torch.full((B, max_l, 2), 77, device=dev, dtype=torch.int32),
               "span_score": torch.full((B, max_l), 7.0, device=dev)}
        out.update({k: torch.full((B, T), 77, device=dev, dtype=torch.int32) for k in FRAME_KEYS})
        args = [None if k == null else out[k] for k in names]
        _lib.call("as_ctc_align", x, x.stride(1), x.stride(0), T_arg, B, C, 0, tg, tg.shape[1], il_d, tl_d, max_l_arg, 0, ws, ws_bytes,
                  out["score"], *args)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    full = call()
    want = run(dev, logp, targets, il, tl)
    for k in ("score", *names):
        assert full[k].tobytes() == want[k].tobytes(), k
    for null in names:
        got = call(null)
        for k in ("score", *names):
            if k == null:
                assert (got[k] == (7.0 if k == "span_score" else 77)).all(), f"{k} was written though NULL"
            else:
                assert got[k].tobytes() == full[k].tobytes(), (null, k)
    with pytest.raises(RuntimeError, match="8193 frames"):
        call(T_arg=8193)
    with pytest.raises(RuntimeError, match="target length 2048"):
        call(max_l_arg=2048)
    with pytest.raises(RuntimeError, match="workspace"):
        call(T_arg=4096, max_l_arg=2047)   # needs a workspace, none given


def _rounded_case(seed):
    rng = np.random.default_rng(seed)
    B, T, C = 6, 80, 45
    tl = [20, 1, 7, 0, 13, 20]
    il = [80, 3, 7, 5, 33, 29]
    targets = [[int(v) for v in rng.integers(1, C, size=n)] for n in tl]
    targets[4][3] = targets[4][2]
    targets[2] = labels_without_repeats(rng, 7, C)   # as many frames as labels
    raw = (3.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    return raw, targets, il, tl


@pytest.mark.parametrize("logits", [False, True])
def test_rounded_inputs_stay_within_the_rounding_bound(dev, logits):
    raw, targets, il, tl = _rounded_case(12)
    if logits:
        x = raw
        logp64 = torch.log_softmax(torch.from_numpy(raw).double(), -1).numpy()
    else:
        x = torch.log_softmax(torch.from_numpy(raw), -1).numpy()   # fp32 log-probabilities, taken as given
        logp64 = x.astype(np.float64)
    got = run(dev, x, targets, il, tl, logits=logits)
    worst = 0.0
    for b in range(len(tl)):
        Tb, tg = il[b], targets[b]
        optimum, _ = F.viterbi(logp64[b, :Tb], tg, 0)
        assert np.isfinite(optimum) and got["feasible"][b]
        states = F.states_from_frame_index(got["frame_index"][b, :Tb])
        assert F.is_valid_path(states, tg, 0), b
        assert (got["frame_index"][b, Tb:] == -1).all()
        M = np.abs(logp64[b, :Tb][np.isfinite(logp64[b, :Tb])]).max()
        bound = (Tb * Tb + 4 * Tb) * M * 2.0 ** -24
        mine = F.rescore(logp64[b, :Tb], tg, 0, states)
        print(f"logits={logits} b={b} Tb={Tb} |score - rescore| = {abs(float(got['score'][b]) - mine):.3e}, "
              f"optimum - rescore = {optimum - mine:.3e}, bound = {bound:.3e}")
        assert abs(float(got["score"][b]) - mine) <= bound
        assert optimum - mine <= 2 * bound
        worst = max(worst, abs(float(got["score"][b]) - mine) / bound)
        fi, ft, ff, spans, span_score = F.expand(states, logp64[b, :Tb], tg, 0, raw.shape[1], max(tl))
        assert np.array_equal(got["frame_token"][b], ft) and np.array_equal(got["frame_filled"][b], ff)
        assert np.array_equal(got["spans"][b], spans)
        ok = ~np.isnan(span_score)
        assert np.array_equal(np.isnan(got["span_score"][b]), ~ok)
        assert (np.abs(got["span_score"][b][ok] - span_score[ok]) <= bound).all()
    assert worst <= 1.0


def test_filled_tokens_reproduce_a_per_frame_truth(dev):
    from artspeech_amd.phoneme_recognition import forced_align
    from artspeech_amd.phoneme_recognition.forced_align import FrameAgreement, filled_tokens
    rng = np.random.default_rng(13)
    B, T, C = 3, 50, 9
    il = [50, 31, 12]
    truth = np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        t = 0
        while t < il[b]:
            n = int(rng.integers(1, 6))
            prev = truth[b, t - 1] if t else -1
            truth[b, t: t + n] = rng.choice([c for c in range(1, C) if c != prev])
            t += n
        truth[b, il[b]:] = -1
    truth_t = torch.from_numpy(truth)
    ctc = [torch.unique_consecutive(truth_t[b, : il[b]]) for b in range(B)]
    tl = [len(c) for c in ctc]
    onehot = torch.nn.functional.one_hot(truth_t.clamp(min=0), C).float()
    em = torch.log(0.9 * onehot + 0.1 / C).to(dev)
    targets = torch.nn.utils.rnn.pad_sequence(ctc, batch_first=True, padding_value=-1).to(dev)
    al = forced_align(em, targets, il, tl)
    assert al.feasible.all()
    tokens = filled_tokens(al, targets).cpu().numpy()
    assert np.array_equal(tokens, truth)
    assert np.array_equal(filled_tokens(al, torch.cat(ctc), tl).cpu().numpy(), truth)
    assert np.array_equal(al.frame_token.cpu().numpy(), truth)   # no blank frame is needed, so none is taken
    metric = FrameAgreement(0, "articulatory_target")   # the fn_metrics call form, on probabilities
    metric.set_truth(truth_t, il)
    assert metric(em.exp(), targets, il, tl) == 1.0
    metric.set_truth(torch.where(truth_t == truth_t[0, 0], truth_t + 1, truth_t), il)   # every frame of one token now disagrees
    assert 0.0 < metric(em.exp(), targets, il, tl) < 1.0
    spans = al.spans.cpu().numpy()
    for b in range(B):
        assert spans[b, 0, 0] == 0 and spans[b, tl[b] - 1, 1] == il[b] and (spans[b, 1: tl[b], 0] == spans[b, : tl[b] - 1, 1]).all()
        segments = al.segments(b, 50.0)
        assert [s[0] for s in segments] == ctc[b].tolist() and segments[-1][2] == il[b] / 50.0
        assert all(abs(s[3] - np.log(0.9 + 0.1 / C)) < 1e-6 for s in segments)


def test_repeats_are_bit_identical(dev):
    raw, targets, il, tl = _rounded_case(14)
    first = run(dev, raw, targets, il, tl, logits=True)
    assert_same_outputs(run(dev, raw, targets, il, tl, logits=True), first)


@pytest.mark.parametrize("logits", [False, True])
def test_a_forbidden_label_makes_the_utterance_infeasible_not_nan(dev, logits):
    rng = np.random.default_rng(15)
    logp = grid(rng, 3, 10, 5)
    logp[0, :, 3] = -np.inf      # utterance 0 needs label 3
    logp[2, 4, :] = -np.inf      # utterance 2: a frame in which nothing is allowed
    got = run(dev, logp, [[1, 3], [1, 3], [2]], [10, 10, 10], [2, 2, 1], logits=logits)
    assert got["score"].tolist()[0] == -np.inf and got["score"][2] == -np.inf and np.isfinite(got["score"][1])
    assert got["feasible"].tolist() == [False, True, False]
    assert (got["frame_index"][[0, 2]] == -1).all() and np.isnan(got["span_score"][[0, 2]]).all()


@pytest.mark.parametrize("config, truth_key", [("align_recognizer_acoustic_synthetic", "acoustic_target"),
                                               ("align_recognizer_synthetic", "articulatory_target")])
def test_align_test_and_the_entry_point_end_to_end(dev, tmp_path, config, truth_key):
    import yaml

    import align_phoneme_recognition as A
    from artspeech_amd.phoneme_recognition import Feature, Target, TrainableDeepSpeech2, align_test
    from torch.utils.data import DataLoader
    from train_phoneme_recognition import Criterion, _make_dataset, build_vocabulary, make_collate_fn
    with open(os.path.join(ROOT, "configs", config + ".yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["seq_dict"] = {"num_sentences": 4}
    vocabulary = build_vocabulary(None, Criterion.CTC)
    torch.manual_seed(0)
    model = TrainableDeepSpeech2(num_classes=len(vocabulary), **cfg["model_params"]).to(dev)
    feature = Feature(cfg["feature"])
    dataset = _make_dataset("synthetic", cfg["database_name"], cfg["seq_dict"], vocabulary, feature, None, cfg["synthetic"], 2)
    loader = DataLoader(dataset, batch_size=4, shuffle=False, collate_fn=make_collate_fn("synthetic", feature, 0, dataset))
    seen = []
    info = align_test(model, loader, Target.CTC, Target(truth_key), feature=feature, device=dev,
                      on_batch=lambda batch, al, first: seen.append((first, al.score.shape[0])))
    assert set(info) == {"frame_agreement", "feasible_fraction", "mean_score_per_frame"} and seen == [(0, 4)]
    assert 0.0 <= info["feasible_fraction"] <= 1.0 and 0.0 <= info["frame_agreement"] <= 1.0
    assert info["mean_score_per_frame"] <= 0.0

    state = tmp_path / "model.pt"
    torch.save(model.state_dict(), state)
    out = A.main(**dict(cfg, state_dict_filepath=str(state), save_dir=str(tmp_path / "out"), seed=0))
    assert set(info) < set(out) and 0.0 <= out["feasible_fraction"] <= 1.0 and 0.0 <= out["frame_agreement"] <= 1.0
    assert (tmp_path / "out" / "info_align.json").exists()
    for index in range(4):
        lines = open(tmp_path / "out" / "alignments" / f"{index}.csv").read().split()
        assert lines[0] == "phoneme,start_frame,end_frame,start_time,end_time,score"
        assert len(lines) - 1 in (0, int(dataset[index]["ctc_target_length"]))   # 0: an utterance without an alignment
        frames = np.load(tmp_path / "out" / "alignments" / f"{index}_frames.npy")
        assert frames.ndim == 1 and (frames >= 0).all() and len(frames) == (int(lines[-1].split(",")[2]) if len(lines) > 1 else 0)
        assert (tmp_path / "out" / "alignments" / f"{index}_phonemes.txt").exists()
