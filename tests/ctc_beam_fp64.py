"""CTC beam search over prefixes restated for the tests (plain Python / numpy in float64, no engine code): the contract that
as_ctc_beam_search is held to, an enumeration of all alignments to check the contract itself, and the emissions the tests use.

A hypothesis is (prefix = the collapsed label sequence so far, ends_in_blank, score); the search starts from ((), False, 0).
Per frame t:

1. shortlist: the K classes with the highest x[t, .], equal values in ascending class index;
2. every live hypothesis (p, f, s) and shortlisted class n contributes s + x[t, n] (+ sil_score if n == sil) to
   (p, True) if n is the blank, to (p, False) if n is p's last label and f is False, to (p + (n,), False) otherwise; -inf is dropped;
3. contributions below best - beam_threshold are dropped (best: the largest single contribution), before merging;
4. contributions with one (prefix, flag) merge by max (log_add False) or logaddexp (True);
5. the beam_size best merged hypotheses stay.

At the end hypotheses with one prefix merge by the same rule; best first, the first nbest.  A length of 0 gives [((), 0.0)]; a
frame whose contributions are all -inf gives [].  Ties between merged scores at a rank boundary are not part of the contract."""
import itertools
import math

import numpy as np

NEG = -math.inf


def scores_of(x, mode):
    """The additive scores of one utterance's rows in float64: "scores" as given, "probs" their log (log(0) = -inf), "logits"
    their row log-softmax."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "probs":
            return np.where(x > 0, np.log(np.where(x > 0, x, 1.0)), NEG)
        if mode == "logits":
            m = x.max(axis=1, keepdims=True)
            lse = m + np.log(np.exp(x - np.where(np.isfinite(m), m, 0.0)).sum(axis=1, keepdims=True))
            return np.where(np.isfinite(x), x - lse, NEG)
    assert mode == "scores", mode
    return x


def _merge(a, b, log_add):
    if not log_add:
        return max(a, b)
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(min(a, b) - m))


def beam_search(x, blank=0, beam_size=50, beam_size_token=None, beam_threshold=50.0, log_add=False, nbest=1, sil=-1, sil_score=0.0,
                stats=None):
    """x (Tb, C) additive scores.  Returns [(labels tuple, score)] best first, at most nbest.  ``stats`` (a dict) receives: "gap",
    the smallest decision gap met (shortlist boundary, threshold, rank beam_size against beam_size + 1, final order over the
    first nbest + 1); "recreated", how often a prefix that had been live and had died came back; "max_rel", the largest
    distance of a live score from its frame's best; "max_abs_x", the largest finite |x|."""
    x = np.asarray(x, dtype=np.float64)
    Tb, C = x.shape
    K = C if beam_size_token is None else int(beam_size_token)
    gap, recreated, max_rel = math.inf, 0, 0.0
    hyps = {((), False): 0.0}
    seen, live = {()}, {()}
    dead = False
    for t in range(Tb):
        row = [float(v) for v in x[t]]
        order = sorted(range(C), key=lambda c: (-row[c], c))
        if K < C and row[order[K]] > NEG:
            gap = min(gap, row[order[K - 1]] - row[order[K]])
        contributions = []
        for (p, f), s in hyps.items():
            for n in order[:K]:
                v = s + row[n] + (sil_score if n == sil else 0.0)
                if not v > NEG:
                    continue
                if n == blank:
                    key = (p, True)
                elif p and n == p[-1] and not f:
                    key = (p, False)
                else:
                    key = (p + (n,), False)
                contributions.append((key, v))
        if not contributions:
            dead = True
            break
        best = max(v for _, v in contributions)
        cut = best - beam_threshold
        merged = {}
        for key, v in contributions:
            if cut > NEG:
                gap = min(gap, abs(v - cut))
            if v >= cut:
                merged[key] = _merge(merged.get(key, NEG), v, log_add)
        ranked = sorted(merged.items(), key=lambda kv: -kv[1])
        if len(ranked) > beam_size:
            gap = min(gap, ranked[beam_size - 1][1] - ranked[beam_size][1])
        hyps = dict(ranked[:beam_size])
        scores = list(hyps.values())
        max_rel = max(max_rel, max(scores) - min(scores))
        now = {p for p, _ in hyps}
        recreated += len([p for p in now - live if p in seen])
        seen |= now
        live = now
    final = {}
    if not dead:
        for (p, _), s in hyps.items():
            final[p] = _merge(final.get(p, NEG), s, log_add)
    ranked = sorted(final.items(), key=lambda kv: -kv[1])
    for (_, a), (_, b) in zip(ranked[:nbest], ranked[1:nbest + 1]):
        gap = min(gap, a - b)
    if stats is not None:
        finite = np.abs(x[np.isfinite(x)])
        stats.update(gap=gap, recreated=recreated, max_rel=max_rel, max_abs_x=float(finite.max()) if finite.size else 0.0)
    return [(p, s) for p, s in ranked[:nbest]]


def margin(Tb, stats):
    """The worst-case float32 accumulation of a relative score over Tb frames: 4 roundings a frame (the emission's log, the
    addition, the merge, the subtraction of the frame's best) of values no larger than max_rel + max|x|."""
    return 4 * Tb * 2.0 ** -24 * (stats["max_rel"] + stats["max_abs_x"])


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def brute_force(x, blank=0, log_add=True):
    """All C^Tb alignments grouped by labelling: [(labels, score)] best first, the score the logsumexp (log_add) or the max of the
    alignments' summed scores.  -inf labellings are left out."""
    x = np.asarray(x, dtype=np.float64)
    Tb, C = x.shape
    groups = {}
    for path in itertools.product(range(C), repeat=Tb):
        s = float(sum(x[t, c] for t, c in enumerate(path)))
        if s > NEG:
            groups.setdefault(collapse(path, blank), []).append(s)
    out = []
    for labels, ss in groups.items():
        m = max(ss)
        out.append((labels, m + math.log(sum(math.exp(s - m) for s in ss)) if log_add else m))
    return sorted(out, key=lambda kv: -kv[1])


def peaky_emissions(rng, T, C, blank=0, mode="scores"):
    """(T, C) float32 recogniser-like rows: normal * 1.5 noise, + 2 on the classes of a run-length labelling (runs of 1 to 4
    frames, blank runs between them).  "scores": their log-softmax; "probs": their softmax; "logits": as they are."""
    z = rng.normal(size=(T, C)) * 1.5
    t = 0
    while t < T:
        c = int(rng.integers(0, C))
        n = int(rng.integers(1, 5))
        z[t:t + n, c] += 2.0
        t += n
    if mode == "logits":
        return z.astype(np.float32)
    lp = z - np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)) - z.max(1, keepdims=True)
    return (np.exp(lp) if mode == "probs" else lp).astype(np.float32)


def peaky_batch(seed, B, T, C, blank=0, mode="scores"):
    """(x (B, T, C) float32, lengths (B,) int64 in [T / 2, T], the first one T) from one seed; the same draws in every mode."""
    rng = np.random.default_rng(seed)
    x = np.stack([peaky_emissions(rng, T, C, blank, mode) for _ in range(B)])
    lengths = rng.integers(T // 2, T + 1, size=B).astype(np.int64)
    lengths[0] = T
    return x, lengths


def decidable(x, lengths, mode, **params):
    """Per utterance: (the oracle's hypotheses, its stats, margin) of a batch; an utterance is compared exactly only when
    stats["gap"] >= margin."""
    out = []
    for b in range(x.shape[0]):
        stats = {}
        hyps = beam_search(scores_of(x[b, : int(lengths[b])], mode), stats=stats, **params)
        out.append((hyps, stats, margin(int(lengths[b]), stats)))
    return out
