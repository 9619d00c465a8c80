"""Metrics of the recogniser (reference ``phoneme_recognition/metrics.py``): ``EditDistance``, torchmetrics'
``word_error_rate`` over the space-joined token strings of the decoded predictions and the targets -- the total word-level
Levenshtein distance divided by the total number of reference words (computed on the host)."""


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
    return errors / total if total else float("inf") if errors else 0.0


def make_pred_and_target_sentences(decoder, emissions, targets, emissions_lengths, targets_lengths):
    """(reference MetricsMixin.make_pred_and_target_sentences) -> (predicted sentences, target sentences) of token indices."""
    emissions, targets = emissions.detach().cpu(), targets.detach().cpu()
    target_sequences = [" ".join(str(int(tok)) for tok in tgt[: int(n)]) for tgt, n in zip(targets, targets_lengths)]
    results = decoder(emissions, emissions_lengths)
    pred_sequences = [" ".join(str(int(tok)) for tok in res[0].tokens) for res in results]
    return pred_sequences, target_sequences


class EditDistance:
    def __init__(self, decoder):
        self.decoder = decoder

    def __call__(self, emissions, targets, emissions_lengths, targets_lengths):
        preds, tgts = make_pred_and_target_sentences(self.decoder, emissions, targets, emissions_lengths, targets_lengths)
        return word_error_rate(preds, tgts)
