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
  (tests/golden/recognizer_eval.npz holds the reference's own results)."""
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
