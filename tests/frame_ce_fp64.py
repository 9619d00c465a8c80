"""Restatements of the frame-level criterion and metrics, the contract of artspeech_amd/csrc/frame_ce.hip and of the four classes
of phoneme_recognition/metrics.py:

* ``cross_entropy``: ``torch.nn.functional.cross_entropy`` in float64 on the CPU over the gathered valid rows -- the reference's
  CrossEntropyLoss.forward (metrics.py:110-120: pad masks, boolean gathers, nn.CrossEntropyLoss) -- with its gradient with
  respect to the full padded (T, B, C) logits from autograd;
* ``auroc_counts``: (n_pos, n_neg, u2) per class by a numpy sort and a walk over the tie groups;
* ``confusion`` / ``accuracy`` / ``f1``: torchmetrics' MulticlassAccuracy / MulticlassF1Score definitions from a confusion matrix."""
import numpy as np
import torch


def valid_mask(lengths, B, T):
    return np.arange(T)[None, :] < np.clip(np.asarray(lengths, dtype=np.int64), 0, T)[:, None]   # (B, T)


def cross_entropy(x, targets, lengths, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0, gout=1.0):
    """x (T, B, C) array-like, targets (B, S >= max length) -> (loss float64, gradient (T, B, C) float64, valid frames that are not
    ignored, sum of their target weights)."""
    x64 = torch.as_tensor(np.asarray(x), dtype=torch.float64).clone().requires_grad_(True)
    T, B, C = x64.shape
    tg = np.asarray(targets, dtype=np.int64)
    if tg.shape[1] < T:
        tg = np.concatenate([tg, np.full((B, T - tg.shape[1]), ignore_index, dtype=np.int64)], axis=1)
    mask = torch.from_numpy(valid_mask(lengths, B, T))
    rows = x64.permute(1, 0, 2)[mask]                       # (N, C): the reference's emissions[pad_mask == 1]
    y = torch.from_numpy(tg[:, :T])[mask]
    w = None if weight is None else torch.as_tensor(np.asarray(weight), dtype=torch.float64)
    loss = torch.nn.functional.cross_entropy(rows, y, weight=w, ignore_index=ignore_index, reduction=reduction,
                                             label_smoothing=label_smoothing)
    (loss * gout).backward()
    kept = y != ignore_index
    den = float((w[y[kept]] if w is not None else torch.ones(int(kept.sum()), dtype=torch.float64)).sum())
    return float(loss.detach()), x64.grad.numpy(), int(kept.sum()), den


def gather_frames(scores, targets, lengths, ignore_index=-100):
    """scores (B, T, C), targets (B, S) -> (scores (N, C), labels (N,)) of the frames t < lengths[b] whose target lies in [0, C)
    and is not ignore_index."""
    scores = np.asarray(scores)
    B, T, C = scores.shape
    tg = np.asarray(targets, dtype=np.int64)
    if tg.shape[1] < T:
        tg = np.concatenate([tg, np.full((B, T - tg.shape[1]), ignore_index, dtype=np.int64)], axis=1)
    tg = tg[:, :T]
    keep = valid_mask(lengths, B, T) & (tg != ignore_index) & (tg >= 0) & (tg < C)
    return scores[keep], tg[keep]


def auroc_counts(scores, labels):
    """scores (N, C) float32, labels (N,) -> int64 (n_pos, n_neg, u2) per class: u2 = sum over the groups of equal score of
    pos_g * (2 * negatives below the group + neg_g)."""
    scores = np.asarray(scores, dtype=np.float32)
    N, C = scores.shape
    n_pos, n_neg, u2 = (np.zeros(C, dtype=np.int64) for _ in range(3))
    for c in range(C):
        pos = labels == c
        n_pos[c], n_neg[c] = int(pos.sum()), int(N - pos.sum())
        order = np.argsort(scores[:, c], kind="stable")
        s, p = scores[order, c], pos[order]
        below = at = 0
        while at < N:
            end = at
            while end < N and s[end] == s[at]:
                end += 1
            pos_g = int(p[at:end].sum())
            neg_g = (end - at) - pos_g
            u2[c] += pos_g * (2 * below + neg_g)
            below += neg_g
            at = end
    return n_pos, n_neg, u2


def auroc(n_pos, n_neg, u2, average="macro"):
    n_pos, n_neg, u2 = (np.asarray(v, dtype=np.float64) for v in (n_pos, n_neg, u2))
    ok = (n_pos > 0) & (n_neg > 0)
    per = np.full(len(u2), np.nan)
    per[ok] = u2[ok] / (2.0 * n_pos[ok] * n_neg[ok])
    if average in ("none", None):
        return per
    if not ok.any():
        return float("nan")
    w = np.ones(int(ok.sum())) if average == "macro" else n_pos[ok]
    return float((per[ok] * w).sum() / w.sum())


def confusion(pred, labels, n):
    cm = np.zeros((n, n), dtype=np.int64)
    for p, t in zip(np.asarray(pred), np.asarray(labels)):
        if 0 <= p < n and 0 <= t < n:
            cm[t, p] += 1
    return cm


def _per_class(cm, f1):
    tp = np.diag(cm).astype(np.float64)
    fp, fn = cm.sum(axis=0) - tp, cm.sum(axis=1) - tp
    num, den = (2 * tp, 2 * tp + fp + fn) if f1 else (tp, tp + fn)
    per = np.zeros(len(tp))
    per[den > 0] = num[den > 0] / den[den > 0]
    return per, tp, fp, fn


def _averaged(cm, average, f1):
    per, tp, fp, fn = _per_class(np.asarray(cm, dtype=np.int64), f1)
    if average in ("none", None):
        return per
    if average == "micro":
        num, den = (2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum()) if f1 else (tp.sum(), tp.sum() + fn.sum())
        return float(num / den) if den else 0.0
    w = (tp + fp + fn > 0).astype(np.float64) if average == "macro" else tp + fn
    return float((per * w).sum() / w.sum()) if w.sum() else 0.0


def accuracy(cm, average="macro"):
    return _averaged(cm, average, f1=False)


def f1(cm, average="macro"):
    return _averaged(cm, average, f1=True)
