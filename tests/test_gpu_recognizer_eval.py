"""The recogniser's evaluation on the device (csrc/recog_eval.hip, phoneme_recognition/align.py): decoding against torch on the host,
the edit distance against the host Levenshtein, the alignment counts against the host restatement of the reference's path and
against the reference's own results (tests/golden/recognizer_eval.npz), the two matrices against that fixture, the metrics against
their host paths, the limits, and train -> test end to end.  Everything is integer work: every comparison is exact, except the
float64 normalisation on the host (1e-12)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

AS_ERR_UNSUPPORTED, AS_ERR_WORKSPACE = -2, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx():
    return load_golden("recognizer_eval")


# ------------------------------------------------------------------------------------------------------------- decoding
T_DEC = 70   # runs of repeats cross the 64-frame boundary


def _decode_case(C, seed):
    """(emissions (6, T, C), lengths) -- 0: long runs over frame 64; 1: all blank; 2: a _ a; 3: exact ties and a NaN; 4: length 0;
    5: length 1."""
    g = torch.Generator().manual_seed(seed)
    em = torch.rand(6, T_DEC, C, generator=g)
    a = C - 1
    em[0, 55:69, a] = 2.0                                   # one run from frame 55 to 68
    em[0, 69, 1] = 2.0
    em[1, :, 0] = 2.0                                       # all blank
    em[2] = 0.0
    em[2, :, 0] = 1.0
    em[2, 0:2, a] = 2.0                                     # a a _ _ a: both a survive
    em[2, 4, a] = 2.0
    em[3, 10, :] = 0.25                                     # every class ties: class 0 wins
    em[3, 11, 1:] = 3.0                                     # classes 1.. tie: class 1 wins
    em[3, 12, [1, a]] = 5.0
    em[3, 13, a] = float("nan")                             # a NaN is the maximum
    em[3, 14, 1] = float("nan")
    em[3, 14, a] = float("nan")                             # two NaNs: the first wins
    em[3, 15, 2] = float("inf")
    return em, torch.tensor([T_DEC, T_DEC, 5, T_DEC, 0, 1])


def _host_decode(em, lengths, blank):
    out = []
    for b in range(em.shape[0]):
        n = em.shape[1] if lengths is None else int(lengths[b])
        raw = torch.argmax(em[b, :n], dim=-1)
        u = torch.unique_consecutive(raw)
        out.append((raw, u[u != blank]))
    return out


def _check_decode(got, want, T):
    tokens, counts, argmax = (t.cpu() for t in got)
    assert tokens.dtype == counts.dtype == argmax.dtype == torch.int32 and tokens.shape == argmax.shape == (len(want), T)
    for b, (raw, u) in enumerate(want):
        assert int(counts[b]) == len(u), (b, int(counts[b]), len(u))
        assert torch.equal(tokens[b, : len(u)].long(), u) and (tokens[b, len(u):] == -1).all(), b
        assert torch.equal(argmax[b, : len(raw)].long(), raw) and (argmax[b, len(raw):] == -1).all(), b


@pytest.mark.parametrize("C", [3, 45, 70])
def test_decode_matches_torch_on_the_host(C, dev):
    from artspeech_amd.phoneme_recognition.align import decode_top1
    em, lengths = _decode_case(C, seed=C)
    want = _host_decode(em, lengths, 0)
    assert len(want[1][1]) == 0 and want[2][1].tolist() == [C - 1, C - 1] and want[3][0][10:16].tolist() == [0, 1, 1, C - 1, 1, 2]
    assert C - 1 in want[0][1].tolist()
    emd = em.to(dev)
    _check_decode(decode_top1(emd, lengths, 0, return_argmax=True), want, T_DEC)
    _check_decode(decode_top1(emd, lengths.to(dev), 0, return_argmax=True), want, T_DEC)            # lengths already on the device
    _check_decode(decode_top1(emd, None, 0, return_argmax=True), _host_decode(em, None, 0), T_DEC)   # every frame
    _check_decode(decode_top1(emd, lengths, -1, return_argmax=True), _host_decode(em, lengths, -1), T_DEC)   # no blank token
    tbc = em.permute(1, 0, 2).contiguous().to(dev)                                                  # the (T, B, C) layout, viewed
    _check_decode(decode_top1(tbc.permute(1, 0, 2), lengths, 0, return_argmax=True), want, T_DEC)
    tokens, counts = decode_top1(emd, lengths, 0)                                                   # without the arg-max output
    assert torch.equal(tokens, decode_top1(emd, lengths, 0, return_argmax=True)[0])


def test_decoders_decode_device_matches_their_host_call(dev):
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder, TopKDecoder
    em, lengths = _decode_case(45, seed=7)
    em[3] = torch.rand(T_DEC, 45, generator=torch.Generator().manual_seed(8))   # no ties: torch.topk leaves their order open
    names = ["<blank>"] + [f"p{i}" for i in range(44)]
    for dec in (GreedyCTCDecoder(names, blank_token="<blank>"), TopKDecoder(names, blank_token=0), TopKDecoder(names)):
        host = dec(em, lengths)
        tokens, counts = dec.decode_device(em.to(dev), lengths)
        for b, hyp in enumerate(host):
            want = [int(t) for t in hyp[0].tokens]
            assert tokens[b, : int(counts[b])].tolist() == want and int(counts[b]) == len(want), (type(dec).__name__, b)


# ------------------------------------------------------------------------------------------- edit distance and alignment
def _random_pairs():
    """About 500 pairs: every L in {0, 1, 63, 64, 65, 130} with every P in {0, 1, 64, 200}, over 2 and 45 tokens, half of them
    correlated (the prediction starts as a copy of the target), plus identical sequences."""
    rng = np.random.default_rng(5)
    pairs = []
    for rep in range(10):
        for V in (2, 45):
            for L in (0, 1, 63, 64, 65, 130):
                for P in (0, 1, 64, 200):
                    tgt = rng.integers(0, V, L)
                    pred = rng.integers(0, V, P)
                    if rep % 2 and L and P:
                        n = min(P, L)
                        pred[:n] = np.where(rng.random(n) < 0.7, tgt[:n], pred[:n])
                    pairs.append((pred.tolist(), tgt.tolist()))
    for L in (1, 63, 64, 65, 130):
        for V in (2, 45):
            seq = rng.integers(0, V, L).tolist()
            pairs.append((seq, list(seq)))
    return pairs


def _pack(seqs, pitch=None):
    pitch = max([len(s) for s in seqs] + [0]) if pitch is None else pitch
    out = torch.full((len(seqs), pitch), -1, dtype=torch.int32)
    for k, s in enumerate(seqs):
        out[k, : len(s)] = torch.tensor(s, dtype=torch.int32)
    return out, torch.tensor([len(s) for s in seqs], dtype=torch.int32)


def _host_counts(pairs, n_classes, class_map=None):
    """The host restatement: substitution_matrix("both") over the class strings."""
    from artspeech_amd.phoneme_recognition.metrics import substitution_matrix
    m = (lambda t: t) if class_map is None else (lambda t: class_map[t])
    preds = [" ".join(str(m(t)) for t in p) for p, _ in pairs]
    tgts = [" ".join(str(m(t)) for t in q) for _, q in pairs]
    return substitution_matrix(preds, tgts, [str(c) for c in range(n_classes)], "both", None).astype(np.int64)


CLASS_MAP = [(7 * t + 3) % 8 for t in range(45)]   # 45 tokens onto 8 classes


@pytest.fixture(scope="module")
def pairs():
    from artspeech_amd.phoneme_recognition.metrics import _levenshtein
    p = _random_pairs()
    return {"pairs": p, "dist": [_levenshtein(a, b) for a, b in p],
            "dist_mapped": [_levenshtein([CLASS_MAP[t] for t in a], [CLASS_MAP[t] for t in b]) for a, b in p],
            "counts": _host_counts(p, 45), "counts_mapped": _host_counts(p, 8, CLASS_MAP)}


def test_edit_distance_matches_the_host_levenshtein(pairs, dev):
    from artspeech_amd.phoneme_recognition.align import edit_distance
    p = pairs["pairs"]
    assert 480 <= len(p) <= 520
    pred, pc = _pack([a for a, _ in p])
    tgt, tc = _pack([b for _, b in p])
    assert pred.shape[1] == 200 and tgt.shape[1] == 130
    got = edit_distance(pred.to(dev), pc.to(dev), tgt.to(dev), tc.to(dev))
    assert got.dtype == torch.int32 and got.tolist() == pairs["dist"]
    assert edit_distance(pred.to(dev), pc, tgt, tc, class_map=CLASS_MAP).tolist() == pairs["dist_mapped"]
    # int64 targets padded with -1 and lengths on the host, as the data loader hands them over
    assert edit_distance(pred.to(dev), pc.to(dev), tgt.long(), tc.long()).tolist() == pairs["dist"]
    # the narrower kernels: one and two 64-column chunks per lane (pitch 63 -> columns 0..63, pitch 65 -> 0..65)
    for pitch in (63, 65):
        idx = [k for k, (_, b) in enumerate(p) if len(b) <= pitch]
        sub_p, sub_pc = _pack([p[k][0] for k in idx])
        sub_t, sub_tc = _pack([p[k][1] for k in idx], pitch)
        assert edit_distance(sub_p.to(dev), sub_pc, sub_t, sub_tc).tolist() == [pairs["dist"][k] for k in idx], pitch
    # an empty side altogether: pitch 0
    none, zero = torch.zeros(3, 0, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    some, n = _pack([[1, 2], [], [3]])
    assert edit_distance(some.to(dev), n, none, zero).tolist() == [2, 0, 1]
    assert edit_distance(none.to(dev), zero, some, n).tolist() == [2, 0, 1]


@pytest.mark.parametrize("L,P", [(300, 100), (700, 90), (2047, 70), (40, 4096)])
def test_edit_distance_wide_tables(L, P, dev):
    """8, 16 and 32 column chunks per lane, and the longest prediction: three pairs each, one of them a corrupted copy."""
    from artspeech_amd.phoneme_recognition.align import edit_distance
    from artspeech_amd.phoneme_recognition.metrics import _levenshtein
    rng = np.random.default_rng(L + P)
    tgts = [rng.integers(0, 3, L).tolist(), rng.integers(0, 45, L - 7).tolist(), rng.integers(0, 45, L).tolist()]
    preds = [rng.integers(0, 3, P).tolist(), rng.integers(0, 45, P).tolist(), None]
    preds[2] = [t for t in tgts[2] if rng.random() < 0.9][:P]
    pred, pc = _pack(preds, P)
    tgt, tc = _pack(tgts, L)
    got = edit_distance(pred.to(dev), pc, tgt, tc).tolist()
    assert got == [_levenshtein(a, b) for a, b in zip(preds, tgts)]


def test_align_counts_match_the_host_substitution_matrix(pairs, dev):
    from artspeech_amd.phoneme_recognition.align import align_counts
    p = pairs["pairs"]
    pred, pc = _pack([a for a, _ in p])
    tgt, tc = _pack([b for _, b in p])
    pred, tgt = pred.to(dev), tgt.to(dev)
    counts, dist = align_counts(pred, pc, tgt, tc, 45)
    assert counts.dtype == torch.int32 and counts.shape == (46, 46)
    assert dist.tolist() == pairs["dist"] and np.array_equal(counts.cpu().numpy(), pairs["counts"])
    assert pairs["counts"][:45, 45].sum() > 0 and pairs["counts"][45, :45].sum() > 0      # deletions and insertions occur
    again, _ = align_counts(pred, pc, tgt, tc, 45)
    assert torch.equal(again, counts)                                                    # repeats are identical
    mapped, dist_m = align_counts(pred, pc, tgt, tc, 8, class_map=CLASS_MAP)
    assert dist_m.tolist() == pairs["dist_mapped"] and np.array_equal(mapped.cpu().numpy(), pairs["counts_mapped"])
    # accumulation over two calls equals one call over the concatenation
    half = len(p) // 2
    acc = torch.zeros(46, 46, dtype=torch.int32, device=dev)
    align_counts(pred[:half], pc[:half], tgt[:half], tc[:half], 45, out=acc)
    out, _ = align_counts(pred[half:], pc[half:], tgt[half:], tc[half:], 45, out=acc)
    assert out is acc and torch.equal(acc, counts)


def test_align_counts_with_the_table_in_the_workspace(dev):
    """(P + 1) (L + 1) uint16 past the workgroup's LDS: the table goes to the workspace and the counts stay the same."""
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition.align import align_counts
    from artspeech_amd.phoneme_recognition.metrics import _levenshtein
    rng = np.random.default_rng(11)
    p = []
    for k, (P, L) in enumerate([(260, 140), (0, 140), (260, 0), (17, 133), (255, 9), (200, 139)]):
        tgt = rng.integers(0, 5, L)
        pred = rng.integers(0, 5, P)
        if k in (0, 5):
            pred[:L] = np.where(rng.random(min(P, L)) < 0.8, tgt[: min(P, L)], pred[:L])
        p.append((pred.tolist(), tgt.tolist()))
    pred, pc = _pack([a for a, _ in p])
    tgt, tc = _pack([b for _, b in p])
    need = _lib.lib().as_align_workspace_bytes(len(p), 260, 140)
    assert need == 2 * len(p) * 261 * 141
    counts, dist = align_counts(pred.to(dev), pc, tgt, tc, 5)
    assert dist.tolist() == [_levenshtein(a, b) for a, b in p]
    assert np.array_equal(counts.cpu().numpy(), _host_counts(p, 5))


@pytest.mark.parametrize("name", ["doc", "v2", "v5", "v12"])
def test_align_counts_reproduce_the_reference_fixture(name, fx, dev):
    from artspeech_amd.phoneme_recognition.align import align_counts
    vocab = [str(s) for s in fx[f"a/{name}/vocab"]]
    preds = [[vocab.index(t) for t in str(s).split()] for s in fx[f"a/{name}/preds"]]
    tgts = [[vocab.index(t) for t in str(s).split()] for s in fx[f"a/{name}/targets"]]
    pred, pc = _pack(preds)
    tgt, tc = _pack(tgts)
    counts, _ = align_counts(pred.to(dev), pc, tgt, tc, len(vocab))
    assert np.array_equal(counts.cpu().numpy(), fx[f"a/{name}/counts"].astype(np.int64))


# --------------------------------------------------------------------------------------------------------- the matrices
def _fixture_batch(fx, dev):
    vocabulary = {str(tok): i for i, tok in enumerate(fx["b/vocab"])}
    return (vocabulary, torch.from_numpy(fx["b/emissions"]).to(dev), torch.from_numpy(fx["b/targets"]), torch.from_numpy(fx["b/lengths"]),
            torch.from_numpy(fx["b/target_lengths"]))


@pytest.mark.parametrize("gtag", ["tokens", "groups"])
def test_substitution_matrix_reproduces_the_reference_fixture(gtag, fx, dev):
    from artspeech_amd.phoneme_recognition import PHONETIC_CLASSES, compute_substitution_matrix
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder, TopKDecoder
    vocabulary, em, targets, lengths, tl = _fixture_batch(fx, dev)
    groups = PHONETIC_CLASSES if gtag == "groups" else None
    best_path = GreedyCTCDecoder(list(vocabulary), blank_token="<blank>")
    topk = TopKDecoder(list(vocabulary), blank_token=0)
    got = compute_substitution_matrix(em, targets.to(dev), lengths, tl, best_path, vocabulary, groups=groups)
    want = fx[f"b/trimmed/{gtag}"]
    assert got.dtype == np.float64 and got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    rows = got.sum(axis=1)
    assert np.all((np.abs(rows - 1) <= 1e-12) | (rows == 0))
    got = compute_substitution_matrix(em, targets, lengths, tl, topk, vocabulary, groups=groups)     # TopKDecoder ignores lengths
    assert np.abs(got - fx[f"b/untrimmed/{gtag}"]).max() <= 1e-12
    # the reference's own call form: lists of per-utterance tensors, the emissions trimmed
    trimmed = [em[b, : int(lengths[b])] for b in range(em.shape[0])]
    got = compute_substitution_matrix(trimmed, list(targets), list(lengths), list(tl), topk, vocabulary, groups=groups)
    assert np.abs(got - want).max() <= 1e-12


def test_confusion_matrix_reproduces_the_reference_fixture(fx, dev):
    from artspeech_amd.phoneme_recognition import PHONETIC_CLASSES, compute_confusion_matrix
    from artspeech_amd.phoneme_recognition.align import decode_top1
    vocabulary, em, _, lengths, _ = _fixture_batch(fx, dev)
    argmax = decode_top1(em, lengths, return_argmax=True)[2]
    valid = torch.arange(em.shape[1])[None, :] < lengths[:, None]
    preds = argmax[valid.to(dev)]                                           # device tensor, utterance after utterance
    tgts = torch.from_numpy(fx["b/frame_targets"])[valid]
    got = compute_confusion_matrix(preds, tgts.to(dev), vocabulary)
    assert got.dtype == np.int64 and np.array_equal(got, fx["c/tokens/counts"])
    got = compute_confusion_matrix(preds.cpu().numpy().astype(np.float32), tgts.numpy(), vocabulary, normalize="true")   # the reference's form
    assert np.abs(got - fx["c/tokens/true"]).max() <= 1e-12
    mask = torch.from_numpy(fx["c/groups/mask"])
    got = compute_confusion_matrix(preds[mask.to(dev)], tgts[mask], vocabulary, groups=PHONETIC_CLASSES)
    assert np.array_equal(got, fx["c/groups/counts"])
    got = compute_confusion_matrix(preds[mask.to(dev)], tgts[mask], vocabulary, groups=PHONETIC_CLASSES, normalize="true")
    assert np.abs(got - fx["c/groups/true"]).max() <= 1e-12
    # with a token outside the groups (<unk>, <blank>) the class "other" = max(groups) + 1 = 7 joins the labels
    got = compute_confusion_matrix(preds, tgts, vocabulary, groups=PHONETIC_CLASSES)
    assert got.shape[0] == fx["c/groups/counts"].shape[0] + 1 and got.sum() == len(tgts)
    assert np.array_equal(got[:-1, :-1], fx["c/groups/counts"])


def test_confusion_counts_padded_batch_and_large_class_count(fx, dev):
    """The (B, T) form run_test uses (lengths, -1 padding) equals the flat form; more classes than the LDS histogram holds."""
    from artspeech_amd.phoneme_recognition.align import confusion_counts, decode_top1
    _, em, _, lengths, _ = _fixture_batch(fx, dev)
    argmax = decode_top1(em, lengths, return_argmax=True)[2]
    frame_targets = torch.from_numpy(fx["b/frame_targets"])
    host = np.zeros((12, 12), dtype=np.int64)
    for b in range(em.shape[0]):
        for t in range(int(lengths[b])):
            host[int(frame_targets[b, t]), int(argmax[b, t])] += 1
    got = confusion_counts(argmax, frame_targets.to(dev), lengths, 12)
    assert np.array_equal(got.cpu().numpy(), host)
    assert np.array_equal(confusion_counts(argmax, frame_targets, None, 12).cpu().numpy(), host)   # the -1 padding is skipped
    short = confusion_counts(argmax, frame_targets[:, :9], lengths, 12)                          # S < T: min(length, T, S) frames
    assert int(short.sum()) == int(lengths.clamp(max=9).sum())
    wide = confusion_counts(argmax, frame_targets, lengths, 100, class_map=[9 * t for t in range(12)], out=None)   # 100 x 100 counters
    assert np.array_equal(wide.cpu().numpy()[::9, ::9], host) and int(wide.sum()) == host.sum()
    confusion_counts(argmax, frame_targets, lengths, 12, out=got)                                # accumulates
    assert np.array_equal(got.cpu().numpy(), 2 * host)


# ---------------------------------------------------------------------------------------------------------- the metrics
def test_metrics_on_the_device_equal_their_host_paths(fx, dev):
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder, TopKDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance, WordInfoLost
    vocabulary, em, targets, lengths, tl = _fixture_batch(fx, dev)
    g = torch.Generator().manual_seed(3)
    B, T, C = 8, 50, 45
    big = torch.softmax(3 * torch.randn(B, T, C, generator=g), -1)
    big_t = torch.randint(2, C, (B, 20), generator=g)
    big_tl = torch.randint(1, 21, (B,), generator=g)
    big_il = torch.randint(1, T + 1, (B,), generator=g)
    for b in range(B):
        big_t[b, big_tl[b]:] = -1
    cases = [(list(vocabulary), em.cpu(), targets, lengths, tl), ([f"t{i}" for i in range(C)], big, big_t, big_il, big_tl)]
    for names, e, t, il, tls in cases:
        for dec in (GreedyCTCDecoder(names, blank_token=names[0]), TopKDecoder(names, blank_token=0)):
            for metric in (EditDistance(dec), WordInfoLost(dec)):
                host = metric(e, t, il, tls)
                got = metric(e.to(dev), t.to(dev), il, tls)
                assert isinstance(got, float) and got == host, (type(metric).__name__, type(dec).__name__, got, host)
                assert 0 < host
    # a decoder without decode_device keeps the host path, GPU emissions or not
    class Foreign:
        def __call__(self, emissions, lengths):
            assert not emissions.is_cuda
            return GreedyCTCDecoder(list(vocabulary), blank_token="<blank>")(emissions, lengths)
    assert EditDistance(Foreign())(em, targets.to(dev), lengths, tl) == EditDistance(GreedyCTCDecoder(list(vocabulary), blank_token="<blank>"))(
        em, targets.to(dev), lengths, tl)


# ------------------------------------------------------------------------------------------------------------ the limits
def test_sizes_past_the_limits_are_refused_before_any_launch(dev):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition import align
    L, lib = _lib, _lib.lib()
    buf = torch.zeros(16, dtype=torch.int32, device=dev)   # never touched: every call below fails its size check first
    f32 = torch.zeros(16, device=dev)
    st = L.stream_ptr()
    p = L.ptr(buf)
    assert lib.as_decode_top1(L.ptr(f32), 0, 0, 1, 8193, 2, None, 0, p, p, None, st) == AS_ERR_UNSUPPORTED
    assert b"8192" in lib.as_last_error()
    for P_max, L_max in ((4097, 4), (4, 2048)):
        assert lib.as_edit_distance(p, P_max, p, p, L_max, p, 1, None, 0, p, st) == AS_ERR_UNSUPPORTED
        assert lib.as_align_counts(p, P_max, p, p, L_max, p, 1, None, 0, 4, p, p, None, 0, st) == AS_ERR_UNSUPPORTED
        assert lib.as_align_workspace_bytes(1, P_max, L_max) == 0
    need = lib.as_align_workspace_bytes(2, 300, 300)
    assert need == 2 * 2 * 301 * 301
    assert lib.as_align_counts(p, 300, p, p, 300, p, 2, None, 0, 4, p, p, p, need - 1, st) == AS_ERR_WORKSPACE
    assert lib.as_align_counts(p, 300, p, p, 300, p, 2, None, 0, 4, p, p, None, 0, st) == AS_ERR_WORKSPACE
    assert str(need).encode() in lib.as_last_error()
    torch.cuda.synchronize()
    assert not buf.any()
    with pytest.raises(ValueError, match="exceeds"):
        align.decode_top1(torch.zeros(1, 8193, 2, device=dev))
    with pytest.raises(ValueError, match="exceeds"):
        align.edit_distance(torch.zeros(1, 4097, dtype=torch.int32, device=dev), [0], torch.zeros(1, 4, dtype=torch.int32), [0])
    with pytest.raises(ValueError, match="exceeds"):
        align.align_counts(torch.zeros(1, 4, dtype=torch.int32, device=dev), [0], torch.zeros(1, 2048, dtype=torch.int32), [0], 4)
    with pytest.raises(ValueError, match="one entry per utterance"):
        align.edit_distance(torch.zeros(2, 4, dtype=torch.int32, device=dev), [0], torch.zeros(2, 4, dtype=torch.int32), [0, 0])
    with pytest.raises(ValueError, match="predictions but"):
        align.edit_distance(torch.zeros(2, 4, dtype=torch.int32, device=dev), [0, 0], torch.zeros(3, 4, dtype=torch.int32), [0, 0, 0])
    with pytest.raises(ValueError, match="lengths must have"):
        align.decode_top1(torch.zeros(2, 4, 3, device=dev), [1])
    # the longest supported utterance decodes
    em = torch.zeros(1, 8192, 3, device=dev)
    em[0, ::2, 1] = 1.0
    em[0, 1::2, 2] = 1.0
    tokens, counts = align.decode_top1(em, None, 0)
    assert int(counts[0]) == 8192 and tokens[0, :4].tolist() == [1, 2, 1, 2]


# ------------------------------------------------------------------------------------------------------------ end to end
def test_train_then_test_writes_the_evaluation_products(dev, tmp_path):
    import test_phoneme_recognition as E
    import train_phoneme_recognition as T
    with open(os.path.join(ROOT, "configs", "train_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    model_params = dict(in_channels=2, num_residual_layers=2, num_rnn_layers=2, rnn_hidden_size=16, num_features=12,
                        adapter_out_features=10, dropout=0.1)
    synthetic = {"min_len": 10, "max_len": 24, "n_articulators": 2, "n_samples": 6}
    train_dir, test_dir = str(tmp_path / "train"), str(tmp_path / "test")
    cfg.update(num_epochs=2, train_seq_dict={"num_sentences": 8}, valid_seq_dict={"num_sentences": 4}, test_seq_dict={"num_sentences": 4},
               results_dir=train_dir, model_params=model_params, synthetic=synthetic, learning_rate=0.01)
    torch.manual_seed(0)
    out = T.main(**cfg)
    for f in ("best_model.pt", "info_test.json", "substitution_matrix.npy", "confusion_matrix.npy"):
        assert os.path.exists(os.path.join(train_dir, f)), f
    with open(os.path.join(ROOT, "configs", "test_recognizer_synthetic.yaml")) as f:
        tcfg = yaml.safe_load(f)
    tcfg.update(seq_dict={"num_sentences": 4}, model_params=model_params, synthetic=synthetic, save_dir=test_dir,
                state_dict_filepath=os.path.join(train_dir, "best_model.pt"))
    info = E.main(**tcfg)
    with open(os.path.join(test_dir, "info_test.json")) as f:
        written = json.load(f)
    assert written == info and set(info) == {"edit_distance", "word_info_lost"}
    # one batch of the same four sentences, the same weights in the frozen scorer: the trainer's closing pass wrote this value
    assert info["edit_distance"] == out["test"]["edit_distance"]
    with open(os.path.join(train_dir, "info_test.json")) as f:
        assert json.load(f)["edit_distance"] == info["edit_distance"]
    subs, conf = np.load(os.path.join(test_dir, "substitution_matrix.npy")), np.load(os.path.join(test_dir, "confusion_matrix.npy"))
    assert subs.shape == (9, 9) and subs.dtype == np.float64   # 7 phonetic groups, "other", and the insertion / deletion line
    rows = subs.sum(axis=1)
    assert np.all((np.abs(rows - 1) <= 1e-12) | (rows == 0)) and abs(rows[7] - 1) <= 1e-12   # the synthetic tokens are all "other"
    assert np.array_equal(conf, [[1.0]])
    assert np.array_equal(subs, np.load(os.path.join(train_dir, "substitution_matrix.npy")))
    assert np.array_equal(conf, np.load(os.path.join(train_dir, "confusion_matrix.npy")))
