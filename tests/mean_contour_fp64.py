"""Float64 yardstick of the phoneme-wise mean contour (NumPy, CPU): run positions, the per-token sample and both forwards, written
from the method's definition -- a frame's run is the maximal stretch of equal consecutive tokens of its utterance around it; the
sample of a token is ``RandomState(random_state).permutation(n)[:round(frac * n)]`` among its n rows in table order; the unweighted
output is the mean of the sampled contours, the weighted one their softmin-weighted mean over |rel_pos_i - rel_pos|.  Independent of
the library (no import of artspeech_amd), used by tests/test_mean_contour_host.py and tests/test_gpu_mean_contour.py."""
from itertools import groupby

import numpy as np


def run_positions(tokens, first_row=None, lengths=None):
    """(abs_pos int64, seq_len int64, rel_pos float64), each (frames,): utterance u = rows first_row[u] .. + lengths[u] of the flat
    token buffer (default: one utterance); frames outside every utterance get 0, 0, 0."""
    tokens = list(np.asarray(tokens).reshape(-1))
    if first_row is None:
        first_row, lengths = [0], [len(tokens)]
    abs_pos, seq_len = np.zeros(len(tokens), np.int64), np.zeros(len(tokens), np.int64)
    for lo, n in zip(first_row, lengths):
        i = int(lo)
        for _, group in groupby(tokens[i:i + int(n)]):
            run = sum(1 for _ in group)
            abs_pos[i:i + run] = np.arange(run)
            seq_len[i:i + run] = run
            i += run
    rel_pos = np.divide(abs_pos, seq_len, out=np.zeros(len(tokens), np.float64), where=seq_len > 0)
    return abs_pos, seq_len, rel_pos


def sample(tokens, token, frac=0.1, random_state=0):
    """the table rows of ``token`` that the sample keeps, in the sample's order"""
    idx = np.flatnonzero(np.asarray(tokens).reshape(-1) == token)
    if frac >= 1.0:
        return idx
    return idx[np.random.RandomState(random_state).permutation(len(idx))[:round(frac * len(idx))]]


class MeanContourYardstick:
    """fit(tokens (n,), rel_pos (n,), contours (n, ...)) keeps the per-token sample in float64; forward(tokens) / forward_weighted(
    tokens, rel_pos) evaluate one utterance.  A token with an empty sample gives NaN."""

    def __init__(self, frac=0.1, random_state=0, dtype=np.float64):
        self.frac, self.random_state, self.dtype = frac, random_state, dtype

    def fit(self, tokens, rel_pos, contours):
        tokens = np.asarray(tokens).reshape(-1)
        contours = np.asarray(contours)
        self.shape = contours.shape[1:]
        self.bank = {}
        for token in np.unique(tokens):
            rows = sample(tokens, token, self.frac, self.random_state)
            self.bank[int(token)] = (np.asarray(rel_pos, self.dtype)[rows], contours[rows].astype(self.dtype))
        return self

    def _rows(self, token):
        rel, x = self.bank.get(int(token), (np.zeros(0, self.dtype), np.zeros((0, *self.shape), self.dtype)))
        return rel, x

    def forward(self, tokens):
        out = np.full((len(tokens), *self.shape), np.nan, self.dtype)
        for i, token in enumerate(tokens):
            _, x = self._rows(token)
            if len(x):
                out[i] = x.mean(axis=0, dtype=self.dtype)
        return out

    def forward_weighted(self, tokens, rel_pos=None):
        if rel_pos is None:
            rel_pos = run_positions(tokens)[2]
        out = np.full((len(tokens), *self.shape), np.nan, self.dtype)
        for i, (token, r) in enumerate(zip(tokens, rel_pos)):
            rel, x = self._rows(token)
            if len(x):
                w = np.exp(-np.abs(rel - self.dtype(r)))
                w = (w / w.sum(dtype=self.dtype)).astype(self.dtype)
                out[i] = np.tensordot(w, x, axes=(0, 0))
        return out


def mean_euclidean(outputs, targets):
    """EuclideanDistance() of (..., 2, N) contours: the mean point distance, float64"""
    d = np.asarray(outputs, np.float64) - np.asarray(targets, np.float64)
    return float(np.sqrt(d[..., 0, :] ** 2 + d[..., 1, :] ** 2).mean())
