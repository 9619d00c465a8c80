"""as_frame_ce_loss / as_frame_ce_grad / as_frame_auroc and the classes over them against the restatements of
tests/frame_ce_fp64.py (float64 ``F.cross_entropy`` over the gathered valid rows; numpy sort and tie groups; confusion-matrix ratios).

The rank statistic, the confusion counts and everything derived from them are integers: every comparison is exact.

The criterion is float32 per frame and float64 across frames.  With u = 2^-24, A = max|x| and w_max = max(1, max w), the kernel
computes per frame m = max x (exact), s = sum_c exp(x_c - m) in [1, C], lse = m + log s and the loss w_y (lse - x_y):
  * x_c - m rounds to within 2 A u, which exp turns into a relative error of s of at most 2 A u; expf adds 2 u per term and
    the C - 1 float32 additions at most (C - 1) u: the relative error of s, hence the absolute error of log s, is at most
    (C + 1 + 2 A) u; logf adds ln(C) u;
  * m + log s rounds to within (A + ln C) u, lse - x_y to within (2 A + ln C) u, the product with w_y to within w_y (2 A + ln C) u:
  |loss - exact| <= w_y (C + 1 + 7 A + 4 ln C) u  <=  w_max (C + 8) (A + ln C + 1) u.
With label smoothing the second term (eps / C) sum_c w_c (lse - x_c) has C summands, each off by at most the same amount and
each at most w_max (2 A + ln C) large, added with at most C u relative rounding: at most eps w_max [(C + 8) + 2 C] (A + ln C + 1) u
more.  Both together, and the two products with (1 - eps) and eps / C, stay below
  bound = 4 w_max (C + 8) (A + ln C + 1) 2^-24        per frame.
The float64 accumulation adds nothing visible, so the sum over n frames is within n bound, the mean (the sum over den = sum w_y)
within n bound / den, plus the one float32 rounding of the returned value.  A gradient element is scale times a bracket whose
only inexact input is p_c = exp(x_c - lse) <= 1, off by at most the error of lse plus the rounding of the difference and of expf
-- below bound / w_max -- and multiplied by at most w_max; so |grad - exact| <= |scale| bound with scale = gout or gout / den."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import frame_ce_fp64 as F
from conftest import ROOT

pytestmark = pytest.mark.gpu

AS_ERR_UNSUPPORTED = -2
U = 2.0 ** -24
ROW_TILE, LOSS_BLOCKS = 16, 256   # frames per workgroup pass and partial sums of as_frame_ce_loss (frame_ce.hip)
EPS = float(np.float32(0.1))      # the label smoothing the kernel sees


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def frame_bound(x, C, weight):
    w_max = max(1.0, float(np.max(weight))) if weight is not None else 1.0
    return 4.0 * w_max * (C + 8) * (float(np.abs(x).max()) + math.log(C) + 1.0) * U


def logits(rng, T, B, C, scale=3.0):
    return (scale * rng.standard_normal((T, B, C))).astype(np.float32)


def labels(rng, B, S, C, pad_from=None, pad=-1):
    tg = rng.integers(0, C, size=(B, S)).astype(np.int64)
    if pad_from is not None:
        for b, n in enumerate(pad_from):
            tg[b, n:] = pad
    return tg


def device_ce(dev, x, tg, lengths, gout=1.0, view=None, **kw):
    """(loss, gradient (T, B, C)) of frame_cross_entropy on the device; view='bt': x is handed over as the permuted view of a
    (B, T, C) tensor."""
    from artspeech_amd.phoneme_recognition import frame_cross_entropy
    if view == "bt":
        base = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev).requires_grad_(True)
        xin = base.permute(1, 0, 2)
        assert not xin.is_contiguous() or min(x.shape[:2]) == 1
    else:
        base = torch.from_numpy(x).to(dev).requires_grad_(True)
        xin = base
    if kw.get("weight") is not None:
        kw["weight"] = torch.from_numpy(np.asarray(kw["weight"], dtype=np.float32)).to(dev)
    loss = frame_cross_entropy(xin, torch.from_numpy(tg).to(dev), torch.as_tensor(lengths), torch.as_tensor(lengths), **kw)
    assert loss.dtype == torch.float32 and loss.shape == ()
    (loss * gout).backward()
    grad = base.grad.cpu().numpy()
    return float(loss.detach()), grad.transpose(1, 0, 2) if view == "bt" else grad


def check_ce(dev, x, tg, lengths, gout=1.0, view=None, **kw):
    """The device result against the oracle, within the bound of the module docstring; figures are printed before they are asserted."""
    T, B, C = x.shape
    reduction = kw.get("reduction", "mean")
    got, grad = device_ce(dev, x, tg, lengths, gout, view, **kw)
    want, gwant, n, den = F.cross_entropy(x, tg, lengths, gout=gout, **kw)
    bound = frame_bound(x, C, kw.get("weight"))
    if n == 0:
        assert (math.isnan(got) and math.isnan(want)) if reduction == "mean" else got == 0.0 == want
        assert np.all(grad == 0)
        return got, grad
    assert den > 0   # the cases keep at least one frame whose class has a weight
    scale = 1.0 / den if reduction == "mean" else 1.0
    loss_bound = n * bound * scale + abs(want) * U
    grad_bound = abs(gout) * scale * bound
    err, gerr = abs(got - want), float(np.abs(grad - gwant).max())
    print(f"T={T} B={B} C={C} {kw}: loss {got:.9g} oracle {want:.9g} err {err:.3g} (bound {loss_bound:.3g}); "
          f"grad err {gerr:.3g} (bound {grad_bound:.3g})")
    assert err <= loss_bound
    assert gerr <= grad_bound
    invalid = ~F.valid_mask(lengths, B, T).T   # (T, B)
    assert np.all(grad[invalid] == 0)
    return got, grad


def some_weights(rng, C):
    if C == 1:
        return np.array([0.5], dtype=np.float32)
    w = rng.uniform(0.25, 2.0, size=C).astype(np.float32)
    w[0] = 0.0
    w[C // 2] = 0.0
    w[C - 1] = 1.5   # at least one class that counts
    return w


# ------------------------------------------------------------------------------------------------------------- criterion
@pytest.mark.parametrize("C", [1, 2, 45, 63, 64, 65, 200])
def test_ce_every_class_width_smoothing_weights_and_reduction(dev, C):
    rng = np.random.default_rng(C)
    T, B = 9, 4
    lengths = [9, 0, 5, 1]   # one utterance of length 0
    x = logits(rng, T, B, C)
    tg = labels(rng, B, T, C, pad_from=lengths)
    tg[:, 0] = C - 1   # the weighted classes occur
    weight = some_weights(rng, C)
    for eps in (0.0, EPS):
        for w in (None, weight):
            for reduction in ("mean", "sum"):
                check_ce(dev, x, tg, lengths, gout=0.7, weight=w, label_smoothing=eps, reduction=reduction, ignore_index=-1)


@pytest.mark.parametrize("T,B,lengths", [(1, 3, [1, 0, 1]), (7, 1, [6]), (1, 1, [1])])
def test_ce_one_frame_and_one_utterance(dev, T, B, lengths):
    rng = np.random.default_rng(T * 10 + B)
    x = logits(rng, T, B, 45)
    tg = labels(rng, B, T, 45)
    tg[:, 0] = 44   # a class with a weight
    check_ce(dev, x, tg, lengths, weight=some_weights(rng, 45), label_smoothing=EPS)
    check_ce(dev, x, tg, lengths, reduction="sum", view="bt")


def test_ce_every_frame_ignored(dev):
    rng = np.random.default_rng(1)
    x = logits(rng, 5, 2, 7)
    tg = np.full((2, 5), -1, dtype=np.int64)
    for lengths, ignore in (([5, 3], -1), ([0, 0], -100)):
        mean, grad = check_ce(dev, x, tg, lengths, ignore_index=ignore, reduction="mean")
        assert math.isnan(mean) and np.all(grad == 0)
        total, grad = check_ce(dev, x, tg, lengths, ignore_index=ignore, reduction="sum")
        assert total == 0.0 and np.all(grad == 0)


def test_ce_target_pitch_and_ignore_index(dev):
    rng = np.random.default_rng(2)
    T, B, C = 11, 3, 45
    lengths = [11, 4, 8]
    x = logits(rng, T, B, C)
    wide = labels(rng, B, T + 6, C, pad_from=lengths)          # pitch S > T, the collate's -1 padding
    check_ce(dev, x, wide, lengths, ignore_index=-1)
    wide[0, 2] = wide[2, 5] = -1                                # ... and -1 inside the lengths: ignored frames
    check_ce(dev, x, wide, lengths, ignore_index=-1, label_smoothing=EPS)
    narrow = labels(rng, B, T, C)
    narrow[0, :3] = 7                                           # an ignore_index inside [0, C)
    got, grad = check_ce(dev, x, narrow, lengths, ignore_index=7, weight=some_weights(rng, C), reduction="sum")
    assert np.all(grad[:3, 0] == 0)
    short = labels(rng, B, 9, C)                                # S < T is fine when S >= max length
    check_ce(dev, x, short, [9, 4, 8])


def test_ce_large_logits_do_not_overflow(dev):
    rng = np.random.default_rng(3)
    T, B, C = 6, 2, 45
    x = rng.uniform(-80.0, 80.0, size=(T, B, C)).astype(np.float32)
    x[0, 0, 0], x[0, 0, 1] = 80.0, -80.0
    tg = labels(rng, B, T, C)
    tg[0, 0] = 1   # the loss of that frame is about 160
    got, _ = check_ce(dev, x, tg, [6, 5], reduction="sum")
    assert math.isfinite(got) and got > 160.0
    check_ce(dev, x, tg, [6, 5], weight=some_weights(rng, C), label_smoothing=EPS)


def test_ce_permuted_view_is_bit_equal_to_its_contiguous_copy(dev):
    rng = np.random.default_rng(4)
    T, B, C = 23, 5, 45
    lengths = [23, 1, 17, 0, 22]
    x = logits(rng, T, B, C)
    tg = labels(rng, B, T, C, pad_from=lengths)
    kw = dict(weight=some_weights(rng, C), label_smoothing=EPS, ignore_index=-1)
    a, ga = device_ce(dev, x, tg, lengths, **kw)
    b, gb = device_ce(dev, x, tg, lengths, view="bt", **dict(kw))
    assert np.float32(a).tobytes() == np.float32(b).tobytes() and ga.tobytes() == np.ascontiguousarray(gb).tobytes()


def raw_loss_and_grad(dev, x, tg, lengths, weight=None, ignore=-100, eps=0.0, mean=1, gout=1.0):
    """The two entry points called directly: (sums (2,) float64, lse (B, T), grad (T, B, C) pre-filled with NaN)."""
    from artspeech_amd import _lib
    T, B, C = x.shape
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(tg).to(dev)
    ld = torch.as_tensor(lengths, dtype=torch.int64).to(dev)
    wd = None if weight is None else torch.from_numpy(weight).to(dev)
    lse = torch.full((B, T), float("nan"), device=dev)
    sums = torch.full((2,), float("nan"), device=dev, dtype=torch.float64)
    nbytes = int(_lib.call("as_frame_ce_workspace_bytes", T, B))
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    _lib.call("as_frame_ce_loss", xd, xd.stride(0), xd.stride(1), T, B, C, td, td.shape[1], ld, wd, ignore, eps, lse, sums, ws, nbytes)
    grad = torch.full((T, B, C), float("nan"), device=dev)
    g = torch.tensor([gout], device=dev)
    _lib.call("as_frame_ce_grad", xd, xd.stride(0), xd.stride(1), T, B, C, td, td.shape[1], ld, wd, ignore, eps, lse, sums, g, mean, grad,
              grad.stride(0), grad.stride(1))
    torch.cuda.synchronize()
    assert int(ws[:8].sum()) == 0   # the ticket is back at zero
    return sums.cpu().numpy(), lse.cpu().numpy(), grad.cpu().numpy()


def test_ce_gradient_buffer_is_fully_written(dev):
    rng = np.random.default_rng(5)
    T, B, C = 10, 3, 45
    lengths = [10, 3, 0]
    x = logits(rng, T, B, C)
    tg = labels(rng, B, T, C)
    tg[0, 4] = -1
    sums, lse, grad = raw_loss_and_grad(dev, x, tg, lengths, ignore=-1)
    assert not np.isnan(grad).any()
    invalid = ~F.valid_mask(lengths, B, T).T
    invalid[4, 0] = True
    assert np.all(grad[invalid] == 0) and np.all(np.abs(grad[~invalid]).sum(axis=-1) > 0)
    want, gwant, n, den = F.cross_entropy(x, tg, lengths, ignore_index=-1)
    assert sums[1] == den == n == 12 and abs(sums[0] / sums[1] - want) <= n * frame_bound(x, C, None) / den
    assert np.abs(grad - gwant).max() <= frame_bound(x, C, None) / den
    ref_lse = torch.logsumexp(torch.from_numpy(x).double(), dim=-1).numpy().T   # (B, T)
    valid = F.valid_mask(lengths, B, T)
    valid[0, 4] = False
    assert np.abs(lse[valid] - ref_lse[valid]).max() <= frame_bound(x, C, None) and np.isnan(lse[~valid]).all()


@pytest.mark.parametrize("rows", [ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, ROW_TILE * LOSS_BLOCKS - 1, ROW_TILE * LOSS_BLOCKS,
                                  ROW_TILE * LOSS_BLOCKS + 1])
def test_ce_frame_counts_around_the_row_tile_and_the_reduction_grid(dev, rows):
    rng = np.random.default_rng(rows)
    C = 5
    x = logits(rng, rows, 1, C)
    tg = labels(rng, 1, rows, C)
    check_ce(dev, x, tg, [rows], weight=some_weights(rng, C), label_smoothing=EPS)
    B = 3   # the same number of valid frames spread over ragged utterances
    lengths = [rows // 2, 0, rows - rows // 2]
    T = max(lengths)
    x = logits(rng, T, B, C)
    check_ce(dev, x, labels(rng, B, T, C), lengths, view="bt")


def test_ce_thesis_shape_repeats_bit_identically(dev):
    rng = np.random.default_rng(6)
    T, B, C = 200, 32, 45
    lengths = rng.integers(60, T + 1, size=B).tolist()
    lengths[0], lengths[1] = T, 0
    x = logits(rng, T, B, C)
    tg = labels(rng, B, T, C, pad_from=lengths)
    kw = dict(weight=some_weights(rng, C), label_smoothing=EPS, ignore_index=-1)
    first = check_ce(dev, x, tg, lengths, view="bt", **dict(kw))
    for _ in range(3):
        again = device_ce(dev, x, tg, lengths, view="bt", **dict(kw))
        assert np.float32(first[0]).tobytes() == np.float32(again[0]).tobytes() and first[1].tobytes() == again[1].tobytes()


def test_ce_class_limit_is_refused_before_any_launch(dev):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition import frame_cross_entropy
    from artspeech_amd.phoneme_recognition.frame_ce import MAX_CLASSES
    rng = np.random.default_rng(7)
    x = logits(rng, 2, 1, MAX_CLASSES)
    check_ce(dev, x, labels(rng, 1, 2, MAX_CLASSES), [2])
    big = torch.zeros(2, 1, MAX_CLASSES + 1, device=dev)
    tg = torch.zeros(1, 2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match=str(MAX_CLASSES)):
        frame_cross_entropy(big, tg, [2], [2])
    ln = torch.tensor([2], device=dev)
    lse, sums, ws = torch.zeros(1, 2, device=dev), torch.zeros(2, device=dev, dtype=torch.float64), torch.zeros(64, device=dev, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=rf"code {AS_ERR_UNSUPPORTED}"):
        _lib.call("as_frame_ce_loss", big, big.stride(0), big.stride(1), 2, 1, MAX_CLASSES + 1, tg, 2, ln, None, -100, 0.0, lse, sums, ws, 64)
    grad, g = torch.zeros_like(big), torch.ones(1, device=dev)
    with pytest.raises(RuntimeError, match=rf"code {AS_ERR_UNSUPPORTED}"):
        _lib.call("as_frame_ce_grad", big, big.stride(0), big.stride(1), 2, 1, MAX_CLASSES + 1, tg, 2, ln, None, -100, 0.0, lse, sums, g, 1,
                  grad, grad.stride(0), grad.stride(1))


def test_cross_entropy_module_matches_the_function_and_trains(dev):
    from artspeech_amd.phoneme_recognition import CrossEntropyLoss
    rng = np.random.default_rng(8)
    T, B, C = 12, 3, 4
    lengths = torch.tensor([12, 7, 9])
    x = logits(rng, T, B, C)
    tg = labels(rng, B, T, C, pad_from=lengths.tolist())
    ce = CrossEntropyLoss(class_weights={"c": 2.0, "a": 0.5, "b": 0.0}, ignore_index=-1, label_smoothing=EPS)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    loss = ce(xd, torch.from_numpy(tg).to(dev), lengths, lengths)
    loss.backward()
    want, gwant, n, den = F.cross_entropy(x, tg, lengths.tolist(), weight=[1.0, 0.5, 0.0, 2.0], ignore_index=-1, label_smoothing=EPS)
    bound = frame_bound(x, C, [2.0])
    assert ce.weight.device == xd.device and abs(float(loss.detach()) - want) <= n * bound / den + abs(want) * U
    assert np.abs(xd.grad.cpu().numpy() - gwant).max() <= bound / den


# ------------------------------------------------------------------------------------------------------------------ AUROC
def grid_scores(rng, B, T, C):
    return (rng.integers(0, 65, size=(B, T, C)) / 64.0).astype(np.float32)


def device_auroc_counts(dev, scores, tg, lengths, ignore=-100):
    from artspeech_amd.phoneme_recognition.frame_ce import frame_auroc_counts
    got = frame_auroc_counts(torch.from_numpy(scores).to(dev), torch.from_numpy(tg).to(dev), torch.as_tensor(lengths), ignore)
    return [v.cpu().numpy() for v in got]


def check_auroc(dev, scores, tg, lengths, ignore=-100):
    got = device_auroc_counts(dev, scores, tg, lengths, ignore)
    want = F.auroc_counts(*F.gather_frames(scores, tg, lengths, ignore))
    for g, w, name in zip(got, want, ("n_pos", "n_neg", "u2")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, g, w)
    return got


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1023, 1025, 2049, 3000])
def test_auroc_counts_on_tied_grids(dev, N):
    rng = np.random.default_rng(N)
    scores = grid_scores(rng, 1, N, 3)
    scores[0, ::7, 1] *= -1.0   # negative scores, and -0 beside +0
    tg = labels(rng, 1, N, 3)
    check_auroc(dev, scores, tg, [N])
    a = device_auroc_counts(dev, scores, tg, [N])
    assert all(np.array_equal(x, y) for x, y in zip(a, device_auroc_counts(dev, scores, tg, [N])))


def test_auroc_degenerate_inputs(dev):
    rng = np.random.default_rng(10)
    flat = np.full((2, 50, 4), 0.25, dtype=np.float32)                          # all scores equal: u2 = n_pos n_neg
    n_pos, n_neg, u2 = check_auroc(dev, flat, labels(rng, 2, 50, 4), [50, 31])
    assert np.array_equal(u2, n_pos * n_neg)
    scores = grid_scores(rng, 1, 40, 2)
    n_pos, n_neg, u2 = check_auroc(dev, scores, np.zeros((1, 40), dtype=np.int64), [40])   # class 0: no negatives; class 1: no positives
    assert n_pos.tolist() == [40, 0] and n_neg.tolist() == [0, 40] and u2.tolist() == [0, 0]
    n_pos, n_neg, u2 = check_auroc(dev, grid_scores(rng, 3, 9, 1), np.zeros((3, 9), dtype=np.int64), [9, 2, 0])   # C = 1
    assert (n_pos[0], n_neg[0], u2[0]) == (11, 0, 0)
    none = check_auroc(dev, grid_scores(rng, 2, 5, 3), np.full((2, 5), -1, dtype=np.int64), [5, 5])   # no valid frame at all
    assert all(not v.any() for v in none)


def test_auroc_ragged_lengths_with_an_ignored_label(dev):
    rng = np.random.default_rng(11)
    B, T, C = 5, 70, 6
    lengths = [70, 0, 33, 1, 64]
    scores = grid_scores(rng, B, T, C)
    tg = labels(rng, B, T + 3, C, pad_from=lengths)   # pitch S > T, -1 padding
    tg[0, 5] = tg[2, 0] = -1                          # outside [0, C): skipped
    check_auroc(dev, scores, tg, lengths)
    tg[4, :10] = 2
    got = check_auroc(dev, scores, tg, lengths, ignore=2)   # an ignored label inside [0, C): class 2 has no positive left
    assert got[0][2] == 0


def test_auroc_thesis_batch_and_the_class(dev):
    from artspeech_amd.phoneme_recognition.metrics import AUROC
    rng = np.random.default_rng(12)
    B, T, C = 32, 200, 45
    lengths = rng.integers(60, T + 1, size=B).tolist()
    lengths[0] = T
    scores = grid_scores(rng, B, T, C)
    tg = labels(rng, B, T, C - 1, pad_from=lengths)   # class 44 never occurs
    n_pos, n_neg, u2 = check_auroc(dev, scores, tg, lengths, ignore=-1)
    assert n_pos[C - 1] == 0
    sd, td, ln = torch.from_numpy(scores).to(dev), torch.from_numpy(tg).to(dev), torch.tensor(lengths)
    per = AUROC(C, average="none")(sd, td, ln, ln)
    assert np.array_equal(per, F.auroc(n_pos, n_neg, u2, "none"), equal_nan=True) and np.isnan(per[C - 1])
    for average in ("macro", "weighted"):
        assert AUROC(C, average)(sd, td, ln, ln) == pytest.approx(F.auroc(n_pos, n_neg, u2, average), abs=1e-14)
    # logits: some lie outside [0, 1], so the class ranks their softmax
    lg = torch.from_numpy(logits(rng, B, T, C)).to(dev)   # (B, T, C)
    on_logits = AUROC(C, None)(lg, td, ln, ln)
    on_probs = AUROC(C, None)(torch.softmax(lg, dim=-1), td, ln, ln)
    assert np.array_equal(on_logits, on_probs, equal_nan=True)
    want = F.auroc(*F.auroc_counts(*F.gather_frames(torch.softmax(lg, dim=-1).cpu().numpy(), tg, lengths, -100)), "none")
    assert np.array_equal(on_probs, want, equal_nan=True)


def test_auroc_frame_limit(dev):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_recognition.frame_ce import MAX_AUROC_FRAMES, frame_auroc_counts
    rng = np.random.default_rng(13)
    B, T, C = 2, MAX_AUROC_FRAMES // 2, 2
    scores = grid_scores(rng, B, T, C)
    tg = labels(rng, B, T, C)
    check_auroc(dev, scores, tg, [T, T])                       # N at the limit
    check_auroc(dev, scores, tg, [T, T - 1])                   # and one below
    sd = torch.from_numpy(grid_scores(rng, 1, MAX_AUROC_FRAMES + 1, C)).to(dev)
    td = torch.zeros(1, MAX_AUROC_FRAMES + 1, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match=str(MAX_AUROC_FRAMES)):   # limit + 1: refused, there is no workspace path
        frame_auroc_counts(sd, td, [MAX_AUROC_FRAMES + 1])
    out = torch.zeros(3, C, dtype=torch.int64, device=dev)
    ln = torch.tensor([MAX_AUROC_FRAMES + 1], device=dev)
    with pytest.raises(RuntimeError, match=rf"code {AS_ERR_UNSUPPORTED}"):
        _lib.call("as_frame_auroc", sd, sd.stride(1), sd.stride(0), MAX_AUROC_FRAMES + 1, 1, C, td, td.shape[1], ln, -100,
                  MAX_AUROC_FRAMES + 1, out[0], out[1], out[2])
    # a padded batch above the limit whose valid frames fit is taken when the lengths are on the host
    check_auroc(dev, sd.cpu().numpy(), td.cpu().numpy(), [100])
    # more valid frames than the caller's bound: refused on the device, every output -1
    _lib.call("as_frame_auroc", sd, sd.stride(1), sd.stride(0), 64, 1, C, td, td.shape[1], torch.tensor([64], device=dev), -100, 10,
              out[0], out[1], out[2])
    assert (out.cpu() == -1).all()


# --------------------------------------------------------------------------------------------------------- accuracy and F1
@pytest.mark.parametrize("absent", [(), (0, 3)])
def test_accuracy_and_f1_equal_the_restatement_from_the_downloaded_argmax(dev, absent):
    from artspeech_amd.phoneme_recognition import decode_top1
    from artspeech_amd.phoneme_recognition.metrics import Accuracy, F1Score
    rng = np.random.default_rng(14)
    B, T, C = 4, 37, 6
    lengths = [37, 12, 0, 30]
    em = grid_scores(rng, B, T, C)   # ties: the lowest index wins, as as_decode_top1 documents
    em[:, :, list(absent)] = -1.0
    present = [c for c in range(C) if c not in absent]
    tg = rng.choice(present, size=(B, T)).astype(np.int64)
    for b, n in enumerate(lengths):
        tg[b, n:] = -1
    ed, td, ln = torch.from_numpy(em).to(dev), torch.from_numpy(tg).to(dev), torch.tensor(lengths)
    argmax = decode_top1(ed, ln, return_argmax=True)[2].cpu().numpy()
    valid = F.valid_mask(lengths, B, T)
    assert np.array_equal(argmax[valid], em.argmax(axis=-1)[valid])
    cm = F.confusion(argmax[valid], tg[valid], C)
    assert cm.sum() == sum(lengths) and all(cm[c].sum() == 0 and cm[:, c].sum() == 0 for c in absent)
    for average in ("macro", "micro", "weighted", "none", None):
        acc, f1 = Accuracy(C, average)(ed, td, ln, ln), F1Score(C, average)(ed, td, ln, ln)
        assert np.array_equal(np.asarray(acc), np.asarray(F.accuracy(cm, average))), average
        assert np.array_equal(np.asarray(f1), np.asarray(F.f1(cm, average))), average
    with pytest.raises(ValueError, match="utterance 1"):
        Accuracy(C)(ed, td, ln, torch.tensor([37, 11, 0, 30]))


# ------------------------------------------------------------------------------------------------------------ end to end
def test_run_epoch_with_the_criterion_and_the_three_metrics(dev):
    from torch.utils.data import DataLoader
    from artspeech_amd.phoneme_recognition import CrossEntropyLoss, Feature, Target, TrainableDeepSpeech2, run_epoch
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    from artspeech_amd.phoneme_recognition.metrics import AUROC, Accuracy, F1Score
    from artspeech_amd.settings import VALID
    from functools import partial
    vocab = {"<unk>": 0, **{f"ph{i:02d}": i + 1 for i in range(8)}}
    C = len(vocab)
    ds = SyntheticPhonemeRecognitionDataset(4, vocab, n_articulators=2, n_samples=6, min_len=10, max_len=24, seed=5, num_special=1)
    loader = DataLoader(ds, batch_size=4, shuffle=False, collate_fn=partial(collate_fn, features_names=[Feature.VOCAL_TRACT]))
    torch.manual_seed(0)
    model = TrainableDeepSpeech2(num_classes=C, in_channels=2, num_residual_layers=1, num_rnn_layers=1, rnn_hidden_size=16,
                                 num_features=12, adapter_out_features=10, dropout=0.1).to(dev)
    metrics = {"accuracy": Accuracy(C), "f1_score": F1Score(C), "auroc": AUROC(C)}
    info = run_epoch(VALID, 1, model, loader, torch.optim.Adam(model.parameters()), CrossEntropyLoss(), False, False,
                     Target.ARTICULATORY, Feature.VOCAL_TRACT, fn_metrics=metrics, device=dev)
    batch = next(iter(loader))
    lengths = batch["vocal_tract_length"].tolist()
    assert lengths == batch["articulatory_target_length"].tolist()
    model.eval()
    with torch.no_grad():
        out = model(batch["vocal_tract"].to(dev), None)   # (B, T, C) logits
    x = out.permute(1, 0, 2).cpu().numpy()
    tg = batch["articulatory_target"].numpy()
    want, _, n, den = F.cross_entropy(x, tg, lengths)
    bound = n * frame_bound(x, C, None) / den + abs(want) * U
    print(f"run_epoch loss {info['loss']:.9g} oracle {want:.9g} (bound {bound:.3g})")
    assert abs(info["loss"] - want) <= bound
    probs = torch.softmax(out, dim=-1).cpu().numpy()
    rows, y = F.gather_frames(probs, tg, lengths)
    cm = F.confusion(rows.argmax(axis=-1), y, C)
    assert info["accuracy"] == F.accuracy(cm) and info["f1_score"] == F.f1(cm)
    assert info["auroc"] == pytest.approx(F.auroc(*F.auroc_counts(rows, y)), abs=1e-14)
    assert all(math.isfinite(v) for v in info.values())


def test_train_frame_recognition_writes_its_products(dev, tmp_path):
    import train_frame_recognition as S
    with open(os.path.join(ROOT, "configs", "train_frame_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    model_params = dict(in_channels=2, num_residual_layers=1, num_rnn_layers=1, rnn_hidden_size=16, num_features=12,
                        adapter_out_features=10, dropout=0.1)
    synthetic = {"min_len": 10, "max_len": 24, "n_articulators": 2, "n_samples": 6, "num_special": 1}
    out_dir = str(tmp_path / "train")
    cfg.update(num_epochs=2, train_seq_dict={"num_sentences": 8}, valid_seq_dict={"num_sentences": 4}, test_seq_dict={"num_sentences": 4},
               results_dir=out_dir, model_params=model_params, synthetic=synthetic, learning_rate=0.01)
    torch.manual_seed(0)
    out = S.main(**cfg)
    for name in ("best_model.pt", "last_model.pt", "checkpoint.pt", "info_test.json"):
        assert os.path.exists(os.path.join(out_dir, name)), name
    with open(os.path.join(out_dir, "info_test.json")) as f:
        written = json.load(f)
    assert written == out["test"] and set(written) == {"loss", "edit_distance", "accuracy", "f1_score", "auroc"}
    assert all(math.isfinite(v) for v in written.values())
    assert len(out["history"]) == 2
    for entry in out["history"]:
        for phase in ("train", "valid"):
            assert set(entry[phase]) == set(written) and all(math.isfinite(v) for v in entry[phase].values())
