"""as_ctc_beam_search / ctc_beam_search on the device against the float64 contract (tests/ctc_beam_fp64.py).

The kernel keeps live scores in float32 relative to the frame's best, so a decision (shortlist boundary, threshold, rank beam_size
against beam_size + 1, final order) whose float64 gap g is below margin = 4 * Tb * 2^-24 * (largest relative live score + max|x|)
-- the worst-case accumulation of four float32 roundings a frame -- may fall either way.  An utterance is compared exactly
(labellings in order, scores within the margin) only when g >= margin; at most 1 in 4 may be skipped, and the seeds were chosen
with the oracle alone so that it stays within that (8/8 decidable at every seed used; other seeds of the same generator gave
6/8 and 7/8; g and the margin are printed).
Wide beams have rank boundaries as close as 1e-6, so they are tested by properties that hold whichever way those fall."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import ctc_beam_fp64 as O
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODES = ("scores", "probs", "logits")
SMALL = {"A": dict(B=8, T=40, C=5, params=dict(beam_size=3, beam_size_token=5, beam_threshold=50.0)),
         "B": dict(B=8, T=60, C=6, params=dict(beam_size=4, beam_size_token=3, beam_threshold=4.0))}   # prunes by shortlist and threshold
WIDE = [dict(B=3, T=150, C=45, beam_size=50), dict(B=2, T=300, C=128, beam_size=64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def search(dev, x, lengths=None, **kwargs):
    from artspeech_amd.phoneme_recognition import ctc_beam_search
    x = torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x
    res = ctc_beam_search(x, lengths, **kwargs)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in ("tokens", "counts", "scores", "num_hyps")}


def hyps_of(out, b, n_classes, blank):
    """[(labels, score)] of utterance b, after checking the layout of its rows: valid non-blank tokens, -1 / 0 / -inf beyond."""
    tokens, counts, scores, found = out["tokens"][b], out["counts"][b], out["scores"][b], int(out["num_hyps"][b])
    assert tokens.dtype == np.int32 and counts.dtype == np.int32 and scores.dtype == np.float32
    hyps = []
    for k in range(tokens.shape[0]):
        n = int(counts[k])
        if k >= found:
            assert n == 0 and scores[k] == -np.inf and np.all(tokens[k] == -1)
            continue
        row = tokens[k, :n]
        assert np.all(tokens[k, n:] == -1) and np.all((row >= 0) & (row < n_classes) & (row != blank))
        assert np.isfinite(scores[k])
        hyps.append((tuple(int(v) for v in row), float(scores[k])))
    return hyps


def assert_same_bytes(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------- 1. brute force on the device
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("T, C, lengths", [(4, 3, [0, 1, 2, 3, 4, 4]), (3, 4, [0, 1, 2, 3, 3, 2]), (6, 2, [0, 1, 3, 4, 5, 6])])
def test_small_cases_equal_the_enumeration_of_all_alignments(dev, seed, T, C, lengths):
    """Nothing is pruned here (the reachable states fit the beam), so the only boundary is the final order: a case would be
    skipped only if two enumerated scores lay closer than the margin, and at these seeds none does (closest pair >= 380 margins)."""
    x, _ = O.peaky_batch(seed, 6, T, C)
    out = search(dev, x, lengths, blank=0, beam_size=64, beam_size_token=C, beam_threshold=math.inf, log_add=True, nbest=64)
    for b, n in enumerate(lengths):
        exact = O.brute_force(x[b, :n].astype(np.float64), 0, log_add=True)
        stats = {}
        O.beam_search(x[b, :n].astype(np.float64), 0, 64, C, math.inf, True, 64, stats=stats)
        margin = O.margin(max(n, 1), stats)
        values = [s for _, s in exact]
        closest = min([a - c for a, c in zip(values, values[1:])], default=math.inf)
        print(f"seed {seed} T {T} C {C} length {n}: closest pair {closest:.3e}, margin {margin:.3e}")
        assert closest >= margin, "a seed for which no case is skipped was to be chosen"
        got = hyps_of(out, b, C, 0)
        assert [p for p, _ in got] == [p for p, _ in exact]
        assert np.abs(np.array([s for _, s in got]) - np.array(values)).max() <= margin
    assert out["num_hyps"][0] == 1 and out["scores"][0, 0] == 0.0 and out["counts"][0, 0] == 0     # length 0: the empty labelling


# ------------------------------------------------------------------ 2. and 3. the contract at small beams, gated by the decision gap
@pytest.mark.parametrize("log_add", [True, False])
@pytest.mark.parametrize("shape, seed", [("A", 3), ("A", 4), ("A", 6), ("B", 1), ("B", 2), ("B", 3)])
def test_small_beams_equal_the_contract(dev, shape, seed, log_add):
    sh = SMALL[shape]
    for mode in MODES:
        x, lengths = O.peaky_batch(seed, sh["B"], sh["T"], sh["C"], 0, mode)
        want = O.decidable(x, lengths, mode, blank=0, log_add=log_add, nbest=3, **sh["params"])
        out = search(dev, x, lengths, blank=0, log_add=log_add, nbest=3, input=mode, **sh["params"])
        if mode == "scores":   # the (T, B, C) tensor of the loss, permuted: a view whose class stride is 1, no copy
            tbc = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev)
            assert_same_bytes(out, search(dev, tbc.permute(1, 0, 2), lengths, blank=0, log_add=log_add, nbest=3, input=mode, **sh["params"]))
        compared = recreated = 0
        for b, (hyps, stats, margin) in enumerate(want):
            recreated += stats["recreated"]
            got = hyps_of(out, b, sh["C"], 0)
            print(f"{shape} seed {seed} log_add {log_add} {mode} utterance {b}: gap {stats['gap']:.3e}, margin {margin:.3e}")
            if stats["gap"] < margin:
                continue
            compared += 1
            assert [p for p, _ in got] == [p for p, _ in hyps], (b, got, hyps)
            assert np.abs(np.array([s for _, s in got]) - np.array([s for _, s in hyps])).max() <= margin, (b, got, hyps)
        assert 4 * compared >= 3 * sh["B"], f"only {compared} of {sh['B']} utterances were decidable"
        assert recreated >= 1, "the shape must make a dead prefix come back"


def test_sil_score_changes_the_result_as_the_contract_says(dev):
    sh = SMALL["A"]
    x, lengths = O.peaky_batch(3, sh["B"], sh["T"], sh["C"])
    plain = search(dev, x, lengths, nbest=3, log_add=True, **sh["params"])
    out = search(dev, x, lengths, nbest=3, log_add=True, sil=1, sil_score=-0.75, **sh["params"])
    assert out["scores"].tobytes() != plain["scores"].tobytes()
    want = O.decidable(x, lengths, "scores", blank=0, log_add=True, nbest=3, sil=1, sil_score=-0.75, **sh["params"])
    compared = 0
    for b, (hyps, stats, margin) in enumerate(want):
        if stats["gap"] < margin:
            continue
        compared += 1
        got = hyps_of(out, b, sh["C"], 0)
        assert [p for p, _ in got] == [p for p, _ in hyps]
        assert np.abs(np.array([s for _, s in got]) - np.array([s for _, s in hyps])).max() <= margin
    assert 4 * compared >= 3 * sh["B"]


# ---------------------------------------------------------------------------------------------------- 4. wide beams by properties
@pytest.fixture(scope="module", params=[0, 1], ids=["C45_beam50", "C128_beam64"])
def wide(request, dev):
    """One batch per shape with both searches run once: shared, and left unchanged, by the tests below."""
    sh = WIDE[request.param]
    x, lengths = O.peaky_batch(11 + request.param, sh["B"], sh["T"], sh["C"])
    xd = torch.from_numpy(x).to(dev)
    runs = {la: search(dev, xd, lengths, beam_size=sh["beam_size"], beam_size_token=sh["C"], nbest=5, log_add=la) for la in (False, True)}
    return sh, x, lengths, xd, runs


def _tolerance(Tb, score):
    return 4 * Tb * 2.0 ** -24 * abs(score)


def test_wide_beam_layout_order_and_distinct_labellings(wide):
    sh, x, lengths, xd, runs = wide
    for out in runs.values():
        for b in range(sh["B"]):
            hyps = hyps_of(out, b, sh["C"], 0)
            assert len(hyps) == 5 == out["num_hyps"][b]
            assert len({p for p, _ in hyps}) == 5
            assert all(a >= c for (_, a), (_, c) in zip(hyps, hyps[1:]))


def test_wide_beam_without_log_add_finds_the_best_path(wide, dev):
    from artspeech_amd.phoneme_recognition import decode_top1
    sh, x, lengths, xd, runs = wide
    tokens, counts = decode_top1(xd, torch.from_numpy(lengths), 0)
    tokens, counts = tokens.cpu().numpy(), counts.cpu().numpy()
    for b in range(sh["B"]):
        n, Tb = int(counts[b]), int(lengths[b])
        assert runs[False]["counts"][b, 0] == n and np.array_equal(runs[False]["tokens"][b, 0, :n], tokens[b, :n])
        best_path = float(x[b, :Tb].astype(np.float64).max(axis=1).sum())
        assert abs(float(runs[False]["scores"][b, 0]) - best_path) <= _tolerance(Tb, best_path)


def test_wide_beam_with_log_add_is_bounded_by_the_ctc_likelihood(wide):
    sh, x, lengths, xd, runs = wide
    out = runs[True]
    logp = torch.from_numpy(x).double().permute(1, 0, 2)
    for b in range(sh["B"]):
        Tb = int(lengths[b])
        hyps = hyps_of(out, b, sh["C"], 0)
        targets = torch.nn.utils.rnn.pad_sequence([torch.tensor(p if p else (1,), dtype=torch.long) for p, _ in hyps], batch_first=True)
        nll = torch.nn.functional.ctc_loss(logp[:, b:b + 1].expand(-1, len(hyps), -1), targets, torch.full((len(hyps),), Tb),
                                           torch.tensor([len(p) for p, _ in hyps]), blank=0, reduction="none")
        for (p, s), exact in zip(hyps, (-nll).tolist()):
            assert s <= exact + _tolerance(Tb, exact), (b, p, s, exact)
        best_path = float(x[b, :Tb].astype(np.float64).max(axis=1).sum())
        assert hyps[0][1] >= best_path - _tolerance(Tb, best_path)


# ------------------------------------------------------------------------------------------------------------- 5. further cases
def test_two_launches_are_bit_identical(wide, dev):
    sh, x, lengths, xd, runs = wide
    for la in (False, True):
        assert_same_bytes(runs[la], search(dev, xd, lengths, beam_size=sh["beam_size"], beam_size_token=sh["C"], nbest=5, log_add=la))


def test_at_the_limits_of_the_supported_range(dev):
    """T = 8192, C = 128, beam 64, all classes shortlisted: half a million trie nodes per utterance, the largest node numbers
    and table, and the relative-score rule over the longest sum.  Without log_add the best hypothesis is still the best path,
    its score the float64 sum of row maxima; with it the best score is no lower."""
    from artspeech_amd.phoneme_recognition import decode_top1
    T, C = 8192, 128
    x, _ = O.peaky_batch(31, 2, T, C)
    lengths = np.array([T, 5001])
    xd = torch.from_numpy(x).to(dev)
    tokens, counts = decode_top1(xd, torch.from_numpy(lengths), 0)
    tokens, counts = tokens.cpu().numpy(), counts.cpu().numpy()
    out = {la: search(dev, xd, lengths, beam_size=64, beam_size_token=C, nbest=2, log_add=la) for la in (False, True)}
    for b in range(2):
        n, Tb = int(counts[b]), int(lengths[b])
        best_path = float(x[b, :Tb].astype(np.float64).max(axis=1).sum())
        assert out[False]["counts"][b, 0] == n and np.array_equal(out[False]["tokens"][b, 0, :n], tokens[b, :n])
        assert np.all(out[False]["tokens"][b, 0, n:] == -1)
        assert abs(float(out[False]["scores"][b, 0]) - best_path) <= _tolerance(Tb, best_path)
        assert float(out[True]["scores"][b, 0]) >= best_path - _tolerance(Tb, best_path)
        for la in (False, True):
            assert len(hyps_of(out[la], b, C, 0)) == 2


def test_nbest_larger_than_the_hypotheses_found(dev):
    x = np.log(np.array([[[0.6, 0.4]], [[0.25, 0.75]]], dtype=np.float32))      # T = 1, C = 2: two hypotheses
    out = search(dev, x, None, nbest=5, log_add=True)
    assert out["tokens"].shape == (2, 5, 1) and list(out["num_hyps"]) == [2, 2]
    assert [p for p, _ in hyps_of(out, 0, 2, 0)] == [(), (1,)] and [p for p, _ in hyps_of(out, 1, 2, 0)] == [(1,), ()]
    np.testing.assert_allclose(out["scores"][:, :2], np.log([[0.6, 0.4], [0.75, 0.25]]), rtol=1e-6)
    assert list(search(dev, x, [0, 1], nbest=2)["num_hyps"]) == [1, 2]


def test_a_row_of_minus_infinity_leaves_no_hypothesis(dev):
    sh = SMALL["A"]
    x, lengths = O.peaky_batch(3, sh["B"], sh["T"], sh["C"])
    plain = search(dev, x, lengths, nbest=3, **sh["params"])
    x = x.copy()
    x[2, 7] = -np.inf
    x[5, int(lengths[5]):] = -np.inf                        # beyond the length: never read
    out = search(dev, x, lengths, nbest=3, **sh["params"])
    assert out["num_hyps"][2] == 0 and hyps_of(out, 2, sh["C"], 0) == []
    keep = [b for b in range(sh["B"]) if b != 2]
    for k in out:
        assert out[k][keep].tobytes() == plain[k][keep].tobytes(), k
    probs = np.exp(x)
    assert search(dev, probs, lengths, nbest=3, input="probs", **sh["params"])["num_hyps"][2] == 0      # log(0) = -inf


def _words(rows):
    return [" ".join(str(int(v)) for v in row) for row in rows]


def test_decoder_feeds_the_metrics_and_both_forms_of_the_substitution_counts(dev):
    from artspeech_amd.phoneme_recognition import align_counts, substitution_counts
    from artspeech_amd.phoneme_recognition.decoders import BeamSearchCTCDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance, WordInfoLost, word_error_rate, word_information_lost
    B, T, C = 6, 50, 7
    x, lengths = O.peaky_batch(21, B, T, C, mode="probs")
    rng = np.random.default_rng(4)
    target_lengths = rng.integers(1, 9, size=B)
    targets = np.full((B, 8), -1, dtype=np.int64)
    for b, n in enumerate(target_lengths):
        targets[b, :n] = rng.integers(1, C, size=n)
    decoder = BeamSearchCTCDecoder(tokens=[f"t{k}" for k in range(C)], blank_token="t0", nbest=3, beam_size=8, log_add=True)
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(targets).to(dev)
    hyps = decoder(xd, lengths)
    assert len(hyps) == B and all(1 <= len(h) <= 3 for h in hyps)
    assert all(h[0].tokens.dtype == torch.int64 and isinstance(h[0].score, float) for h in hyps)
    assert all(a.score >= c.score for h in hyps for a, c in zip(h, h[1:]))
    tokens, counts = decoder.decode_device(xd, lengths)
    assert tokens.shape == (B, T) and tokens.dtype == torch.int32 and counts.shape == (B,)
    for b in range(B):
        assert tokens[b, : int(counts[b])].tolist() == hyps[b][0].tokens.tolist()
    preds, wanted = _words(h[0].tokens.tolist() for h in hyps), _words(targets[b, :n] for b, n in enumerate(target_lengths))
    assert EditDistance(decoder)(xd, td, lengths, target_lengths) == word_error_rate(preds, wanted)
    assert WordInfoLost(decoder)(xd, td, lengths, target_lengths) == word_information_lost(preds, wanted)
    class_map = torch.arange(C, dtype=torch.int32, device=dev)
    direct = align_counts(tokens, counts, td, torch.from_numpy(target_lengths), C, class_map)[0]
    as_tensor = substitution_counts(xd, td, lengths, target_lengths, decoder, class_map, C)
    as_lists = substitution_counts([xd[b, : int(lengths[b])] for b in range(B)], [td[b, :n] for b, n in enumerate(target_lengths)],
                                   lengths, target_lengths, decoder, class_map, C)
    assert torch.equal(as_tensor, direct) and torch.equal(as_lists, direct) and int(direct.sum()) > 0


def test_recording_decoder_searches_a_batch_once_and_keeps_its_n_best(dev):
    from decode_phoneme_recognition import RecordingBeamDecoder
    B, T, C = 4, 30, 6
    x, lengths = O.peaky_batch(22, B, T, C, mode="probs")
    names = [f"t{k}" for k in range(C)]
    decoder = RecordingBeamDecoder(tokens=names, blank_token="t0", nbest=3, beam_size=8, log_add=True)
    xd = torch.from_numpy(x).to(dev)
    first = decoder.decode_device(xd, lengths)
    again = decoder.decode_device(xd, [int(n) for n in lengths])
    assert len(decoder.batches) == 1 and torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    other = xd.clone()
    decoder.decode_device(other, lengths)
    decoder.decode_device(other, lengths - 1)        # other lengths: another search
    assert len(decoder.batches) == 3
    want = decoder(xd, lengths)                       # the plain decoder's host form of the same search
    got = decoder.hypotheses()
    assert len(got) == 3 * B
    for b in range(B):
        assert [h["tokens"] for h in got[b]] == [[names[int(k)] for k in h.tokens] for h in want[b]]
        assert [h["score"] for h in got[b]] == [h.score for h in want[b]]
        assert first[0][b, : int(first[1][b])].tolist() == want[b][0].tokens.tolist()
    # what consumes decode_device gets the same from the one nbest = 3 search as from the plain decoder's nbest = 1 search
    from artspeech_amd.phoneme_recognition import align_counts, edit_distance, substitution_counts
    from artspeech_amd.phoneme_recognition.decoders import BeamSearchCTCDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance, WordInfoLost
    plain = BeamSearchCTCDecoder(tokens=names, blank_token="t0", nbest=3, beam_size=8, log_add=True)
    targets = torch.from_numpy(np.random.default_rng(5).integers(1, C, size=(B, 6))).to(dev)
    target_lengths = [6, 3, 1, 5]
    assert first[0].is_contiguous() and first[1].is_contiguous()
    for metric in (EditDistance, WordInfoLost):
        assert metric(decoder)(xd, targets, lengths, target_lengths) == metric(plain)(xd, targets, lengths, target_lengths)
    class_map = torch.arange(C, dtype=torch.int32, device=dev)
    assert torch.equal(substitution_counts(xd, targets, lengths, target_lengths, decoder, class_map, C),
                       substitution_counts(xd, targets, lengths, target_lengths, plain, class_map, C))
    # and a strided counts view (one column of the (B, nbest) counts) is read as what it holds
    res = plain.search(xd, lengths)
    tl = torch.tensor(target_lengths)
    assert torch.equal(edit_distance(res.tokens[:, 0], res.counts[:, 0], targets, tl),
                       edit_distance(res.tokens[:, 0].contiguous(), res.counts[:, 0].contiguous(), targets, tl))
    assert torch.equal(align_counts(res.tokens[:, 1], res.counts[:, 1], targets, tl, C)[0],
                       align_counts(res.tokens[:, 1].contiguous(), res.counts[:, 1].contiguous(), targets, tl, C)[0])


def _fresh_model_config(tmp_path, name):
    from artspeech_amd.phoneme_recognition import Criterion, DeepSpeech2
    from train_phoneme_recognition import build_vocabulary
    with open(os.path.join(ROOT, "configs", name)) as f:
        cfg = yaml.safe_load(f)
    model_params = dict(in_channels=2, num_residual_layers=2, num_rnn_layers=2, rnn_hidden_size=16, num_features=12,
                        adapter_out_features=10, dropout=0.1)
    torch.manual_seed(0)
    model = DeepSpeech2(num_classes=len(build_vocabulary(None, Criterion.CTC)), **model_params)
    path = str(tmp_path / "fresh_model.pt")
    torch.save(model.state_dict(), path)
    cfg.update(seq_dict={"num_sentences": 4}, model_params=model_params, state_dict_filepath=path,
               synthetic={"min_len": 10, "max_len": 24, "n_articulators": 2, "n_samples": 6})
    return cfg


def test_main_with_the_beam_config_writes_info_and_hypotheses(dev, tmp_path):
    import decode_phoneme_recognition as E
    cfg = _fresh_model_config(tmp_path, "test_recognizer_beam_synthetic.yaml")
    cfg["save_dir"] = str(tmp_path / "beam")
    info = E.main(**cfg)
    with open(os.path.join(cfg["save_dir"], "info_test.json")) as f:
        assert json.load(f) == info and set(info) == {"edit_distance", "word_info_lost"}
    with open(os.path.join(cfg["save_dir"], "hypotheses.json")) as f:
        hyps = json.load(f)
    assert len(hyps) == 4
    for utterance in hyps:
        assert 1 <= len(utterance) <= cfg["decoder"]["nbest"]
        assert all(set(h) == {"tokens", "score"} and all(isinstance(t, str) for t in h["tokens"]) for h in utterance)
        assert all(a["score"] >= c["score"] for a, c in zip(utterance, utterance[1:]))
    assert os.path.exists(os.path.join(cfg["save_dir"], "substitution_matrix.npy"))
    # the metrics are taken on the best hypothesis: asking for one hypothesis only gives the same numbers
    one = E.main(**dict(cfg, save_dir=None, decoder=dict(cfg["decoder"], nbest=1)))
    assert json.dumps(one, sort_keys=True) == json.dumps(info, sort_keys=True)


def test_main_without_a_decoder_key_is_the_greedy_pass(dev, tmp_path):
    """decode_phoneme_recognition.main without a decoder is test_phoneme_recognition.main: the same numbers and files."""
    import decode_phoneme_recognition as E
    import test_phoneme_recognition as today
    cfg = _fresh_model_config(tmp_path, "test_recognizer_synthetic.yaml")
    assert "decoder" not in cfg
    cfg["save_dir"] = str(tmp_path / "plain")
    plain = E.main(**cfg)
    assert not os.path.exists(os.path.join(cfg["save_dir"], "hypotheses.json"))
    assert today.main(**dict(cfg, save_dir=str(tmp_path / "today"))) == plain
    for f in ("info_test.json", "substitution_matrix.npy", "confusion_matrix.npy"):
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "today" / f, "rb").read(), f
    named = E.main(**dict(cfg, save_dir=str(tmp_path / "named"), decoder={"name": "greedy"}))
    assert plain == named and set(plain) == {"edit_distance", "word_info_lost"}
    for f in ("substitution_matrix.npy", "confusion_matrix.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "named" / f))
    # the beam search with max-merging and its best hypothesis alone is best-path decoding: the same numbers by another kernel
    beam = E.main(**dict(cfg, save_dir=None, decoder={"name": "beam", "beam_size": 16}))
    assert beam == plain
