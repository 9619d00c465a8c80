"""CTC forced alignment restated for the tests (numpy, no engine code): the max-plus recursion over the extended label sequence
(S = 2L + 1 states; even states blank, odd state s the label targets[(s - 1) / 2]; moves stay, step, skip between different
labels; start in state 0 or 1, end in S - 1 or S - 2), its tie rules, the trace-back, the spans, the blank-absorbing fill and a
float64 rescoring of any path.  ``dtype`` is the arithmetic of the recursion: float64 is the oracle, float32 restates the kernel's
own accumulation (time order, one addition per step).

Tie rules: candidates in the order stay, step, skip, a later one replaces the best so far only if strictly greater; at the end
the label state S - 2 wins when it is >= state S - 1."""
import numpy as np


def viterbi(logp, targets, blank, dtype=np.float64):
    """logp (Tb, C) log-probabilities of the utterance's own frames, targets a sequence of L labels.  Returns (score, states):
    the path's log-probability in `dtype` and the state of every frame, or (-inf, None) when no alignment exists; (0, []) for
    Tb == 0 == L."""
    logp = np.asarray(logp)
    targets = [int(v) for v in targets]
    Tb, L = logp.shape[0], len(targets)
    S = 2 * L + 1
    if Tb == 0:
        return (dtype(0.0), []) if L == 0 else (dtype(-np.inf), None)
    ext = [blank if s % 2 == 0 else targets[s // 2] for s in range(S)]
    skip = [s % 2 == 1 and s >= 2 and ext[s] != ext[s - 2] for s in range(S)]
    ext, skip = np.asarray(ext), np.asarray(skip)
    neg = dtype(-np.inf)
    a = np.full(S, neg, dtype=dtype)
    a[: min(S, 2)] = logp[0, ext[: min(S, 2)]].astype(dtype)
    back = np.zeros((Tb, S), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tb):
            step = np.concatenate([[neg], a[:-1]]).astype(dtype)
            skp = np.where(skip, np.concatenate([[neg, neg], a[:-2]])[:S], neg).astype(dtype)
            best, bp = a, np.zeros(S, dtype=np.int8)
            m = step > best
            best, bp = np.where(m, step, best), np.where(m, 1, bp)
            m = skip & (skp > best)
            best, bp = np.where(m, skp, best), np.where(m, 2, bp)
            a = (best + logp[t, ext].astype(dtype)).astype(dtype)
            back[t] = bp
    s, best = S - 1, a[S - 1]
    if S >= 2 and a[S - 2] >= best:
        s, best = S - 2, a[S - 2]
    if not best > neg:
        return dtype(-np.inf), None
    states = [0] * Tb
    for t in range(Tb - 1, 0, -1):
        states[t] = s
        s -= int(back[t, s])
    states[0] = s
    return best, states


def rescore(logp, targets, blank, states):
    """The float64 log-probability of a path given as the state of every frame."""
    logp = np.asarray(logp, dtype=np.float64)
    total = 0.0
    for t, s in enumerate(states):
        total += logp[t, blank if s % 2 == 0 else int(targets[s // 2])]
    return total


def states_from_frame_index(frame_index):
    """The state sequence that a frame_index row (entry per frame, -1 on blank frames) stands for: a blank frame sits in the
    blank state after the last emitted entry."""
    states, last = [], -1
    for j in frame_index:
        j = int(j)
        if j >= 0:
            last = j
            states.append(2 * j + 1)
        else:
            states.append(2 * (last + 1))
    return states


def is_valid_path(states, targets, blank):
    """Monotone, legal moves only, legal first and last state: such a path collapses to the target."""
    targets = [int(v) for v in targets]
    S = 2 * len(targets) + 1
    if not states:
        return len(targets) == 0
    if states[0] not in (0, 1) or states[0] >= S or states[-1] not in (S - 1, S - 2) or states[-1] < 0:
        return False
    for p, s in zip(states[:-1], states[1:]):
        d = s - p
        if d not in (0, 1, 2) or s >= S:
            return False
        if d == 2 and not (s % 2 == 1 and targets[s // 2] != targets[s // 2 - 1]):
            return False
    tokens = [blank if s % 2 == 0 else targets[s // 2] for s in states]   # the CTC collapse: merge repeats, then drop blanks
    collapsed = [tok for k, tok in enumerate(tokens) if tok != blank and (k == 0 or tok != tokens[k - 1])]
    return collapsed == targets


def expand(states, logp, targets, blank, T, max_l):
    """The kernel's outputs for one utterance from its path (None: no alignment): frame_index, frame_token, frame_filled [T],
    spans [max_l][2], span_score [max_l] (float64 mean of the label's log-probability over its frames)."""
    targets = [int(v) for v in targets]
    L = len(targets)
    fi, ft, ff = (np.full(T, -1, dtype=np.int32) for _ in range(3))
    spans = np.full((max_l, 2), -1, dtype=np.int32)
    span_score = np.full(max_l, np.nan, dtype=np.float64)
    if states is None:
        return fi, ft, ff, spans, span_score
    logp = np.asarray(logp, dtype=np.float64)
    last = -1
    for t, s in enumerate(states):
        if s % 2 == 1:
            last = s // 2
            fi[t], ft[t] = last, targets[last]
        else:
            ft[t] = blank
        ff[t] = -1 if L == 0 else max(last, 0)   # leading blanks belong to entry 0
    t = 0
    while t < len(states):   # one run of equal states at a time: a state's frames are contiguous on a monotone path
        e = t
        while e < len(states) and states[e] == states[t]:
            e += 1
        if states[t] % 2 == 1:
            j = states[t] // 2
            assert spans[j][0] == -1, "a state's frames are contiguous"
            spans[j] = (t, e)
            span_score[j] = float(np.mean(logp[t:e, targets[j]]))
        t = e
    return fi, ft, ff, spans, span_score


def align_batch(logp, targets, input_lengths, target_lengths, blank, dtype=np.float64):
    """The whole output of forced_align for a (B, T, C) batch of log-probabilities and padded (B, >= max L) targets, as numpy
    arrays: dict(score [B] in `dtype`, states (list per utterance), frame_index, frame_token, frame_filled [B][T], spans
    [B][max L][2], span_score [B][max L] float64)."""
    logp = np.asarray(logp)
    B, T, _ = logp.shape
    max_l = int(max(target_lengths)) if B else 0
    out = dict(score=np.zeros(B, dtype=dtype), states=[], frame_index=np.zeros((B, T), np.int32), frame_token=np.zeros((B, T), np.int32),
               frame_filled=np.zeros((B, T), np.int32), spans=np.zeros((B, max_l, 2), np.int32), span_score=np.zeros((B, max_l)))
    for b in range(B):
        Tb, L = int(input_lengths[b]), int(target_lengths[b])
        tg = [int(v) for v in np.asarray(targets[b])[:L]]
        score, states = viterbi(logp[b, :Tb], tg, blank, dtype)
        out["score"][b] = score
        out["states"].append(states)
        (out["frame_index"][b], out["frame_token"][b], out["frame_filled"][b], out["spans"][b],
         out["span_score"][b]) = expand(states, logp[b, :Tb], tg, blank, T, max_l)
    return out
