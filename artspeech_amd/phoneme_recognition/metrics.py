"""Metrics of the recogniser (reference ``phoneme_recognition/metrics.py``).

* ``EditDistance``: torchmetrics' ``word_error_rate`` over the decoded predictions and the targets -- the total word-level
  Levenshtein distance divided by the total number of reference words.
* ``WordInfoLost``: torchmetrics' ``word_information_lost``, ``1 - (H / N_target) * (H / N_pred)`` with
  ``H = sum max(len_pred, len_target) - sum distance``, written from its documentation (torchmetrics is absent here: parity
  unpinned).

Both take the device path when the emissions are on the GPU and the decoder has ``decode_device``: the decode (as_decode_top1)
and the distances (as_edit_distance) run there, the integer sums are reduced there and one small copy reaches the host, where the
same ratio of the same integers gives the same Python float as the host path.  CPU tensors and foreign decoders take the host
path: decode per utterance, Levenshtein in Python.

* ``edit_matrix`` / ``compute_transitions`` / ``substitution_matrix``: the reference's string-level alignment API (:200-392) on the
  host.  The reference finds its path with a best-first walk over the edit table (``shortest_path``, :218-270); that walk ends on
  the back-trace that steps, from the corner, to the predecessor with the smallest table entry -- ties to the diagonal, then to the
  previous prediction row, then to the previous target column -- which is what is built here and in as_align_counts
  (tests/golden/recognizer_eval.npz holds the reference's own results).

* ``CrossEntropyLoss``, ``Accuracy``, ``F1Score``, ``AUROC``: the frame-level criterion and metrics of the reference's ``loss: CE``
  branch (:87-120, :155-197), one target per frame.  The criterion runs on as_frame_ce_loss / as_frame_ce_grad (frame_ce.py);
  Accuracy and F1 are ratios of the confusion counts of the device's per-frame arg-max (as_decode_top1, as_confusion_counts),
  the AUROC of the rank statistic as_frame_auroc counts.  The emissions stay on the device: a handful of integers is
  downloaded and divided on the host in float64, as ``normalize_counts`` does.  Two departures from torch / torchmetrics:
  ``reduction="none"`` is not built, and a class without a positive or a negative frame is NaN in the AUROC's per-class vector
  and left out of its averages."""
import json
import os

import numpy as np
import torch


def _levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[-1]


def word_error_rate(preds, target):
    """torchmetrics.functional.word_error_rate for lists of strings."""
    errors = total = 0
    for p, t in zip(preds, target):
        pw, tw = p.split(), t.split()
        errors += _levenshtein(pw, tw)
        total += len(tw)
    return _wer(errors, total)


def _wer(errors, total):
    return errors / total if total else float("inf") if errors else 0.0


def _wil(errors, longest, n_target, n_pred):
    """1 - (H / N_target) (H / N_pred), H = longest - errors; IEEE division (an empty side gives nan or -inf, as tensors would)."""
    with np.errstate(all="ignore"):
        h = np.float64(longest - errors)
        return float(1.0 - (h / np.float64(n_target)) * (h / np.float64(n_pred)))


def word_information_lost(preds, target):
    """torchmetrics.functional.word_information_lost for lists of strings (from its documentation; parity unpinned)."""
    errors = longest = n_target = n_pred = 0
    for p, t in zip(preds, target):
        pw, tw = p.split(), t.split()
        errors += _levenshtein(pw, tw)
        longest += max(len(pw), len(tw))
        n_target += len(tw)
        n_pred += len(pw)
    return _wil(errors, longest, n_target, n_pred)


def make_pred_and_target_sentences(decoder, emissions, targets, emissions_lengths, targets_lengths):
    """(reference MetricsMixin.make_pred_and_target_sentences) -> (predicted sentences, target sentences) of token indices."""
    emissions, targets = emissions.detach().cpu(), targets.detach().cpu()
    target_sequences = [" ".join(str(int(tok)) for tok in tgt[: int(n)]) for tgt, n in zip(targets, targets_lengths)]
    results = decoder(emissions, emissions_lengths)
    pred_sequences = [" ".join(str(int(tok)) for tok in res[0].tokens) for res in results]
    return pred_sequences, target_sequences


def _on_device(decoder, emissions):
    return torch.is_tensor(emissions) and emissions.is_cuda and hasattr(decoder, "decode_device")


def _device_sums(decoder, emissions, targets, emissions_lengths, targets_lengths):
    """(sum distance, sum max(len_pred, len_target), sum len_target, sum len_pred) as Python ints: one (4,) copy to the host."""
    from .align import edit_distance
    dev = emissions.device
    tokens, counts = decoder.decode_device(emissions, emissions_lengths)
    targets = torch.as_tensor(targets).to(dev)
    tl = torch.as_tensor(targets_lengths).reshape(-1).to(device=dev, dtype=torch.int32).clamp(0, targets.shape[1])
    dist = edit_distance(tokens, counts, targets, tl)
    sums = torch.stack([dist.sum(), torch.maximum(counts, tl).sum(), tl.sum(), counts.sum()])
    return [int(v) for v in sums.tolist()]


class EditDistance:
    def __init__(self, decoder):
        self.decoder = decoder

    def __call__(self, emissions, targets, emissions_lengths, targets_lengths):
        if _on_device(self.decoder, emissions):
            errors, _, total, _ = _device_sums(self.decoder, emissions, targets, emissions_lengths, targets_lengths)
            return _wer(errors, total)
        preds, tgts = make_pred_and_target_sentences(self.decoder, emissions, targets, emissions_lengths, targets_lengths)
        return word_error_rate(preds, tgts)


class WordInfoLost:
    def __init__(self, decoder):
        self.decoder = decoder

    def __call__(self, emissions, targets, emissions_lengths, targets_lengths):
        if _on_device(self.decoder, emissions):
            return _wil(*_device_sums(self.decoder, emissions, targets, emissions_lengths, targets_lengths))
        preds, tgts = make_pred_and_target_sentences(self.decoder, emissions, targets, emissions_lengths, targets_lengths)
        return word_information_lost(preds, tgts)


# ------------------------------------------------------------------------------------------ frame-level classification
def _ce_arguments(weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
    """nn.CrossEntropyLoss's own arguments, positional or by name."""
    if size_average is not None or reduce is not None:
        raise NotImplementedError("CrossEntropyLoss: the deprecated size_average / reduce arguments are not taken; use reduction")
    return weight, int(ignore_index), reduction, float(label_smoothing)


class CrossEntropyLoss(torch.nn.Module):
    """The reference's CE criterion (metrics.py:87-120): ``nn.CrossEntropyLoss(*args, weight=..., **kwargs)`` over the valid frames
    of a padded batch, on the kernels of frame_ce.py (loss, division and gradient on the device, no boolean gathers).

    ``class_weights`` is a {token name: weight} dict or the path of a JSON file that holds one.  The weight vector is
    ``[1.0] + [w for _, w in sorted(class_weights.items())]``: 1.0 for the unknown class at index 0, then the weights SORTED BY
    TOKEN NAME, not by vocabulary index -- exactly the reference's order, so it fits a vocabulary whose tokens are listed in
    name order.  The remaining arguments are nn.CrossEntropyLoss's (``ignore_index``, ``reduction``, ``label_smoothing``; ``weight``
    only without class_weights, as in the reference, where giving both is a TypeError).  ``reduction="none"`` is not built."""

    def __init__(self, *args, class_weights=None, **kwargs):
        super().__init__()
        if class_weights is not None:
            if "weight" in kwargs:
                raise TypeError("CrossEntropyLoss: got multiple values for keyword argument 'weight' (class_weights sets it)")
            if isinstance(class_weights, (str, os.PathLike)):
                with open(class_weights) as f:
                    class_weights = json.load(f)
            kwargs["weight"] = torch.tensor([1.0] + [w for _, w in sorted(class_weights.items(), key=lambda t: t[0])])
        weight, self.ignore_index, self.reduction, self.label_smoothing = _ce_arguments(*args, **kwargs)
        if self.reduction == "none":
            raise NotImplementedError("CrossEntropyLoss: reduction='none' is not built (the reference never asks for it)")
        if self.reduction not in ("mean", "sum"):
            raise ValueError(f"CrossEntropyLoss: unknown reduction {self.reduction!r}")
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32))

    def forward(self, emissions, targets, emissions_lengths, targets_lengths):
        """emissions (T, B, C) (raw logits in the reference's CE branch), targets (B, S), one per frame."""
        from .frame_ce import frame_cross_entropy
        if self.weight is not None and self.weight.device != emissions.device:
            self.weight = self.weight.to(emissions.device)   # once: the module follows its input
        return frame_cross_entropy(emissions, targets, emissions_lengths, targets_lengths, self.weight, self.ignore_index,
                                   self.reduction, self.label_smoothing)


_AVERAGES = ("macro", "micro", "weighted", "none", None)


def accuracy_from_counts(cm, average="macro"):
    """torchmetrics' MulticlassAccuracy from confusion counts cm[target, prediction], in float64: per-class accuracy is recall
    tp / (tp + fn) (0 without support); macro is its mean over the classes with tp + fp + fn > 0, weighted its support-weighted
    mean, micro sum(tp) / sum(cm); none / None the per-class vector (0 for a class that never occurs)."""
    return _average(*_class_counts(cm), average, lambda tp, fp, fn: (tp, tp + fn))


def f1_from_counts(cm, average="macro"):
    """torchmetrics' MulticlassF1Score from confusion counts, in float64: per class 2 tp / (2 tp + fp + fn) (0 when that is 0 / 0);
    the averages as in accuracy_from_counts."""
    return _average(*_class_counts(cm), average, lambda tp, fp, fn: (2 * tp, 2 * tp + fp + fn))


def _class_counts(cm):
    cm = np.asarray(cm, dtype=np.int64)
    tp = np.diag(cm)
    return tp, cm.sum(axis=0) - tp, cm.sum(axis=1) - tp


def _average(tp, fp, fn, average, ratio):
    if average not in _AVERAGES:
        raise ValueError(f"average must be one of 'macro', 'micro', 'weighted', 'none' or None, got {average!r}")
    with np.errstate(all="ignore"):
        if average == "micro":
            num, den = ratio(tp.sum(), fp.sum(), fn.sum())
            return float(np.float64(num) / np.float64(den)) if den else 0.0
        num, den = ratio(tp, fp, fn)
        per_class = np.where(den > 0, num.astype(np.float64) / np.maximum(den, 1), 0.0)
        if average in ("none", None):
            return per_class
        weights = (tp + fp + fn > 0).astype(np.float64) if average == "macro" else (tp + fn).astype(np.float64)
        return float((per_class * weights).sum() / weights.sum()) if weights.sum() else 0.0


def auroc_from_counts(n_pos, n_neg, u2, average="macro"):
    """One-vs-rest AUROC from as_frame_auroc's integers, in float64: per class u2 / (2 n_pos n_neg), NaN for a class without a
    positive or without a negative frame; macro is the mean over the other classes, weighted their n_pos-weighted mean (NaN if
    there is none); none / None the per-class vector."""
    if average not in ("macro", "weighted", "none", None):
        raise ValueError(f"AUROC: average must be one of 'macro', 'weighted', 'none' or None, got {average!r}")
    n_pos, n_neg, u2 = (np.asarray(v, dtype=np.int64) for v in (n_pos, n_neg, u2))
    with np.errstate(all="ignore"):
        per_class = u2.astype(np.float64) / (2.0 * n_pos.astype(np.float64) * n_neg.astype(np.float64))
    per_class[(n_pos == 0) | (n_neg == 0)] = np.nan
    if average in ("none", None):
        return per_class
    keep = ~np.isnan(per_class)
    weights = keep.astype(np.float64) if average == "macro" else np.where(keep, n_pos, 0).astype(np.float64)
    if not weights.sum():
        return float("nan")
    return float((np.where(keep, per_class, 0.0) * weights).sum() / weights.sum())


def _frame_confusion(emissions, targets, emissions_lengths, targets_lengths, num_classes):
    """The (num_classes, num_classes) confusion counts [target, arg-max] of the valid frames, counted on the device
    (as_decode_top1's arg-max: the lowest index among equal scores, a NaN is the maximum; as_confusion_counts), downloaded once."""
    from .align import confusion_counts, decode_top1
    from .frame_ce import check_frame_lengths
    lengths = check_frame_lengths("frame metrics", emissions_lengths, targets_lengths, emissions.shape[0], emissions.shape[1])
    argmax = decode_top1(emissions, lengths, return_argmax=True)[2]
    return confusion_counts(argmax, targets, lengths, num_classes).cpu().numpy()


class Accuracy:
    """The reference's Accuracy (metrics.py:170-182, torchmetrics' MulticlassAccuracy) from the device's confusion counts of the
    per-frame arg-max; emissions (B, T, C) on the device.  See accuracy_from_counts for the averages."""

    def __init__(self, num_classes, average="macro"):
        if average not in _AVERAGES:
            raise ValueError(f"Accuracy: unknown average {average!r}")
        self.num_classes, self.average = int(num_classes), average

    def __call__(self, emissions, targets, emissions_lengths, targets_lengths):
        return accuracy_from_counts(_frame_confusion(emissions, targets, emissions_lengths, targets_lengths, self.num_classes), self.average)


class F1Score:
    """The reference's F1Score (metrics.py:155-167, torchmetrics' MulticlassF1Score), as Accuracy; see f1_from_counts."""

    def __init__(self, num_classes, average="macro"):
        if average not in _AVERAGES:
            raise ValueError(f"F1Score: unknown average {average!r}")
        self.num_classes, self.average = int(num_classes), average

    def __call__(self, emissions, targets, emissions_lengths, targets_lengths):
        return f1_from_counts(_frame_confusion(emissions, targets, emissions_lengths, targets_lengths, self.num_classes), self.average)


class AUROC:
    """The reference's AUROC (metrics.py:185-197, torchmetrics' MulticlassAUROC with exact thresholds): one-vs-rest, from the rank
    statistic as_frame_auroc counts on the device; emissions (B, T, C) on the device.  If a score of a valid frame lies outside
    [0, 1] the emissions go through ``torch.softmax`` first (torchmetrics' rule).  A class without a positive or without a
    negative frame is NaN in the per-class vector and left out of the averages -- this project's rule (auroc_from_counts)."""

    def __init__(self, num_classes, average="macro"):
        if average not in ("macro", "weighted", "none", None):
            raise ValueError(f"AUROC: unknown average {average!r}")
        self.num_classes, self.average = int(num_classes), average

    def __call__(self, emissions, targets, emissions_lengths, targets_lengths):
        from .frame_ce import check_frame_lengths, frame_auroc_counts
        B, T, Cn = emissions.shape
        if Cn != self.num_classes:
            raise ValueError(f"AUROC: emissions of {Cn} classes, num_classes is {self.num_classes}")
        lengths = check_frame_lengths("AUROC", emissions_lengths, targets_lengths, B, T)
        emissions = emissions.detach()
        if emissions.numel():
            valid = (torch.arange(T)[None, :] < lengths[:, None]).to(emissions.device)
            lo, hi = torch.aminmax(emissions.masked_fill(~valid[:, :, None], 0.5))
            if bool((lo < 0) | (hi > 1)):
                emissions = torch.softmax(emissions, dim=-1)
        counts = torch.stack(frame_auroc_counts(emissions, targets, lengths)).cpu().numpy()
        return auroc_from_counts(*counts, self.average)


# ------------------------------------------------------------------------------------------ the string-level alignment API
def edit_matrix(prediction_tokens, reference_tokens):
    """The edit-distance table, (len(prediction) + 1) rows by (len(reference) + 1) columns (reference :200-215)."""
    P, L = len(prediction_tokens), len(reference_tokens)
    dp = [[0] * (L + 1) for _ in range(P + 1)]
    for i in range(P + 1):
        dp[i][0] = i
    for j in range(L + 1):
        dp[0][j] = j
    for i in range(1, P + 1):
        for j in range(1, L + 1):
            dp[i][j] = min(dp[i - 1][j] + 1, dp[i][j - 1] + 1, dp[i - 1][j - 1] + (prediction_tokens[i - 1] != reference_tokens[j - 1]))
    return dp


def _alignment_path(dp):
    """The path from (0, 0) to the corner: walked back from the corner to the predecessor with the smallest entry, ties to the
    diagonal, then to (i - 1, j), then to (i, j - 1)."""
    i, j = len(dp) - 1, len(dp[0]) - 1
    path = [(i, j)]
    big = float("inf")
    while i > 0 or j > 0:
        d = dp[i - 1][j - 1] if i > 0 and j > 0 else big
        u = dp[i - 1][j] if i > 0 else big
        l = dp[i][j - 1] if j > 0 else big
        if d <= u and d <= l:
            i, j = i - 1, j - 1
        elif u <= l:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return path[::-1]


def compute_transitions(preds, target):
    """Per (prediction, target) pair of space-separated token strings: (deletions, insertions, substitutions) along the
    alignment path in path order -- deletions as target positions, insertions as prediction positions, substitutions (matches
    included) as (target position, prediction position) (reference :273-321)."""
    if isinstance(preds, str):
        preds = [preds]
    if isinstance(target, str):
        target = [target]
    all_transitions = []
    for pred, tgt in zip(preds, target):
        path = _alignment_path(edit_matrix(pred.split(), tgt.split()))
        deletions, insertions, substitutions = [], [], []
        for (ci, cj), (ni, nj) in zip(path[:-1], path[1:]):
            if ci == ni:
                deletions.append(cj)
            elif cj == nj:
                insertions.append(ci)
            else:
                substitutions.append((cj, ci))
        all_transitions.append((deletions, insertions, substitutions))
    return all_transitions


def substitution_matrix(preds, target, vocab, insertions_and_deletions=None, normalize=None):
    """The (len(vocab) + 1)-square float64 matrix of the reference (:324-392): [target token, predicted token] counts of the
    diagonal moves (the main diagonal holds the correct transcriptions), the deletions of a target token in the last column
    (insertions_and_deletions "deletions" or "both"), the insertions of a predicted token in the last row ("insertions" or
    "both"); normalize "true" / "pred" / "all" divides by the row sums / column sums / total, NaN -> 0."""
    if isinstance(preds, str):
        preds = [preds]
    if isinstance(target, str):
        target = [target]
    index = {}
    for k, token in enumerate(vocab):
        index.setdefault(token, k)   # list.index: the first occurrence
    include_insertions = insertions_and_deletions in ("insertions", "both")
    include_deletions = insertions_and_deletions in ("deletions", "both")
    cm = np.zeros((len(vocab) + 1, len(vocab) + 1))
    for pred, tgt, (deletions, insertions, substitutions) in zip(preds, target, compute_transitions(preds, target)):
        pred, tgt = pred.split(), tgt.split()
        for i, j in substitutions:
            cm[index[tgt[i]], index[pred[j]]] += 1
        if include_deletions:
            for i in deletions:
                cm[index[tgt[i]], -1] += 1
        if include_insertions:
            for j in insertions:
                cm[-1, index[pred[j]]] += 1
    return normalize_counts(cm, normalize)


def normalize_counts(cm, normalize=None):
    """The closing step of substitution_matrix (:383-390) in float64: row ("true"), column ("pred") or total ("all") division, NaN -> 0."""
    cm = np.asarray(cm, dtype=np.float64)
    with np.errstate(all="ignore"):
        if normalize == "true":
            cm = cm / cm.sum(axis=1, keepdims=True)
        elif normalize == "pred":
            cm = cm / cm.sum(axis=0, keepdims=True)
        elif normalize == "all":
            cm = cm / cm.sum()
        cm = np.nan_to_num(cm)
    return cm
