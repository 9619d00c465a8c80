"""Phoneme-wise mean contour on MI355X (reference: phoneme_to_articulation/phoneme_wise_mean_contour/__init__.py), the baseline
row of the thesis' result tables.

The reference keeps every training frame in a pandas table (token[, abs_pos, seq_len, rel_pos], one contour per articulator) and,
for EVERY output frame, draws ``df[df.token == token].sample(frac=0.1, random_state=0)`` again and averages the sampled contours:
plainly (``forward_mean_contour``, :125-145) or with softmin weights over ``|rel_pos_i - rel_pos|`` (``forward_weighted_mean_contour``,
:86-122), ``rel_pos`` being the frame's position inside its run of equal tokens divided by the run's length.  The sample depends on
the token alone, so here it is drawn ONCE per token (``sample_rows``: NumPy's generator, the very rows pandas selects), the sampled
frames are compacted into a device-resident bank in CSR form by token, and a batch is evaluated by one launch
(artspeech_amd/csrc/mean_contour.hip): a table look-up, or a kernel regression over the bank -- attention with scalar keys and a
token-equality mask.  There is no CPU path.

``PhonemeWiseMeanContour`` is the model; ``train`` / ``test`` / ``forward_mean_contour`` / ``forward_weighted_mean_contour`` keep the
reference's function surface with the model in place of the DataFrame.  ``SyntheticSegmentedArtSpeechDataset`` yields utterances
with phoneme runs, which the per-frame tokens of ``SyntheticArtSpeechDataset`` do not have.
"""
import ast
import csv
import json
import logging
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
from torch.utils.data import Dataset

from ... import _lib
from ...settings import DATASET_CONFIG, UNKNOWN

POSITION_COLUMNS = ("abs_pos", "seq_len", "rel_pos")


# ---------------------------------------------------------------------------------------------------- host side: the sample
def sample_rows(tokens, vocab_size, frac=0.1, random_state=0, sort=True):
    """The rows ``df[df.token == v].sample(frac=frac, random_state=random_state)`` selects, for every token id v < vocab_size.

    tokens: (n,) integer ids in table order.  pandas draws ``RandomState(random_state).permutation(n_v)[:round(frac * n_v)]`` among
    the n_v rows of the token in table order (``round``: Python's, half to even -- n_v <= 5 at frac = 0.1 is an empty sample).
    Returns (rows int64 grouped by token, offsets int64 (vocab_size + 1,)); inside a token the rows are ascending (``sort``) or in
    pandas' order.  frac >= 1 keeps every row.  O(n log n) once."""
    tokens = np.asarray(tokens).astype(np.int64).reshape(-1)
    order = np.argsort(tokens, kind="stable")
    sorted_tokens = tokens[order]
    lo = np.searchsorted(sorted_tokens, np.arange(vocab_size), side="left")
    hi = np.searchsorted(sorted_tokens, np.arange(vocab_size), side="right")
    rows, offsets = [], np.zeros(vocab_size + 1, np.int64)
    for v in range(vocab_size):
        idx = order[lo[v]:hi[v]]
        n = len(idx)
        if frac < 1.0 and n:
            idx = idx[np.random.RandomState(random_state).permutation(n)[:round(frac * n)]]
            if sort:
                idx = np.sort(idx)
        rows.append(idx)
        offsets[v + 1] = offsets[v] + len(idx)
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int64), offsets


def require_bank(offsets, token_ids, vocabulary=None):
    """Raises IndexError naming the tokens among ``token_ids`` that have no bank row: ids outside the vocabulary, tokens the
    training data never held and tokens whose sample is empty (the reference fails on them inside ``torch.stack``)."""
    offsets = np.asarray(offsets)
    names = {i: t for t, i in (vocabulary or {}).items()}
    bad = []
    for v in sorted({int(t) for t in np.asarray(token_ids).reshape(-1)}):
        if v < 0 or v >= len(offsets) - 1 or offsets[v + 1] == offsets[v]:
            bad.append(f"{names[v]!r} (id {v})" if v in names else f"id {v}")
    if bad:
        raise IndexError("phoneme-wise mean contour: no stored frame for token(s) " + ", ".join(bad) +
                         " (outside the vocabulary, absent from the training data, or an empty sample: round(frac * n) = 0)")


def write_table(path, tokens, positions, contours, articulators):
    """The reference's table file, as ``pd.DataFrame(data).to_csv(index=False)`` writes it (:155-157): ``token[, abs_pos, seq_len,
    rel_pos]`` and one stringified ``[[x...], [y...]]`` list per articulator.  tokens: strings; positions: (rows, 2) integers
    (abs_pos, seq_len) or None; contours (rows, articulators, 2, n_samples) float32."""
    contours = np.asarray(contours, np.float32)
    with open(path, "w", newline="") as f:
        writer = csv.writer(f, lineterminator="\n")
        writer.writerow(["token", *(POSITION_COLUMNS if positions is not None else ()), *articulators])
        for k, token in enumerate(tokens):
            row = [token]
            if positions is not None:
                a, n = int(positions[k][0]), int(positions[k][1])
                row += [a, n, repr(a / n)]
            row += [str(contours[k, i].tolist()) for i in range(len(articulators))]
            writer.writerow(row)
    return path


def read_table(path):
    """A table file -> {"tokens": list of strings, "positions": (rows, 2) int64 or None, "contours": (rows, articulators, 2,
    n_samples) float32, "articulators": the contour columns in file order}.  Parsed with ``csv`` and ``json`` /
    ``ast.literal_eval``: no pandas, no ``eval``."""
    csv.field_size_limit(min(sys.maxsize, 2 ** 31 - 1))
    tokens, pos, contours = [], [], []
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = next(reader, None)
        if not header or header[0] != "token":
            raise ValueError(f"{path}: the first column must be 'token', got {header[:1] if header else header}")
        has_pos = all(c in header for c in POSITION_COLUMNS)
        articulators = [c for c in header[1:] if c not in POSITION_COLUMNS]
        col = {c: i for i, c in enumerate(header)}
        for row in reader:
            if not row:
                continue
            tokens.append(row[0])
            if has_pos:
                pos.append((int(row[col["abs_pos"]]), int(row[col["seq_len"]])))
            contours.append([_parse_list(row[col[a]]) for a in articulators])
    if not tokens:
        raise ValueError(f"{path}: the table holds no rows")
    contours = np.asarray(contours, dtype=np.float32)
    if contours.ndim != 4 or contours.shape[2] != 2:
        raise ValueError(f"{path}: contours {contours.shape}: expected (rows, articulators, 2, n_samples)")
    return {"tokens": tokens, "positions": np.asarray(pos, np.int64) if has_pos else None, "contours": contours,
            "articulators": articulators}


def _parse_list(text):
    try:
        return json.loads(text)
    except ValueError:
        return ast.literal_eval(text)


def token_runs(tokens, first_row, lengths):
    """``_calculate_tokens_lengths_and_positions`` (:19-29) for every frame of a flat device buffer: (abs_pos int32, seq_len int32,
    rel_pos float32), each (frames,).  tokens (frames,) int64 on the device; utterance u = rows first_row[u] .. + lengths[u]."""
    _lib.require_gpu(tokens, "tokens")
    tokens = tokens.contiguous()
    frames, dev = tokens.numel(), tokens.device
    first = torch.as_tensor(first_row, dtype=torch.int64).reshape(-1)
    lens = torch.as_tensor(lengths, dtype=torch.int32).reshape(-1)
    if first.numel() != lens.numel():
        raise ValueError(f"{first.numel()} first rows for {lens.numel()} lengths")
    if first.device.type == "cpu" and lens.device.type == "cpu" and first.numel():
        ends = first + lens
        if bool((lens < 0).any()) or bool((first[1:] < ends[:-1]).any()) or int(first[0]) < 0 or int(ends.max()) > frames:
            raise ValueError("utterances must be ascending, disjoint and inside the token buffer")
    first, lens = first.to(dev), lens.to(dev)
    abs_pos = torch.empty(frames, dtype=torch.int32, device=dev)
    seq_len = torch.empty_like(abs_pos)
    rel_pos = torch.empty(frames, dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(_lib.call("as_token_runs_workspace_ints", frames)), 1), dtype=torch.int32, device=dev)
    _lib.call("as_token_runs", tokens, first, lens, first.numel(), frames, abs_pos, seq_len, rel_pos, ws)
    return abs_pos, seq_len, rel_pos


# ---------------------------------------------------------------------------------------------------- the model
class PhonemeWiseMeanContour:
    """The fitted table of the method.

    After ``fit`` (or ``from_csv`` / ``load_state_dict``), on the device: ``bank`` (M, A, 2, N) float32, the stored frames grouped by
    token id (``offsets`` (V + 1,) int64, CSR) and in data-set order inside a token; ``rel_pos`` (M,) float32 and ``positions`` (M, 2)
    int32 (abs_pos, seq_len) of those frames (``None`` for a table without positions); ``rows`` (M,) int64, each frame's row in the
    table it was drawn from; ``table`` (V, A, 2, N) float32, the per-token mean (NaN for a token without frames).  ``sampled``: the
    bank is a ``frac`` < 1 sample of its table."""

    # The out-of-bank check reads a device flag.  Default: forward() reads it right after its launch (one synchronisation); a loop
    # that synchronises anyway sets ``defer_token_check = True`` and calls ``check_tokens()`` (the encoder-decoder models' switch).
    defer_token_check = False

    def __init__(self, vocabulary=None, articulators=None, n_samples=50):
        self.vocabulary = dict(vocabulary) if vocabulary is not None else None
        self.articulators = list(articulators) if articulators is not None else None
        self.n_samples = int(n_samples)
        self.bank = self.rel_pos = self.positions = self.rows = self.offsets = self.table = None
        self.sampled = False
        self._pending = []

    # ------------------------------------------------------------------------------------------------ fitting
    @property
    def vocab_size(self):
        return int(self.offsets.numel()) - 1

    @property
    def row_elems(self):
        return len(self.articulators) * 2 * self.n_samples

    def _build(self, src, src_rel, src_pos, src_rows, tokens_host, vocab_size, frac, random_state):
        """bank <- the per-token sample of the table src (n, A, 2, N) whose row i holds token tokens_host[i]"""
        dev = src.device
        rows_host, offsets_host = sample_rows(tokens_host, vocab_size, frac, random_state)
        present = np.bincount(np.asarray(tokens_host, np.int64), minlength=vocab_size)[:vocab_size]
        empty = [v for v in range(vocab_size) if present[v] and offsets_host[v + 1] == offsets_host[v]]
        if empty:
            names = {i: t for t, i in (self.vocabulary or {}).items()}
            logging.warning("phoneme-wise mean contour: empty sample (round(%g * n) = 0) for %s", frac,
                            ", ".join(f"{names.get(v, v)!r} (n = {present[v]})" for v in empty))
        M, D = len(rows_host), self.row_elems
        rows = torch.from_numpy(rows_host).to(dev)
        self.offsets = torch.from_numpy(offsets_host).to(dev)
        self._offsets_host = offsets_host
        bank = torch.empty((M, len(self.articulators), 2, self.n_samples), dtype=torch.float32, device=dev)
        rel = torch.zeros(M, dtype=torch.float32, device=dev)
        table = torch.empty((vocab_size, *bank.shape[1:]), dtype=torch.float32, device=dev)
        has_pos = src_rel is not None
        src = src.contiguous()
        src_rel = src_rel.contiguous() if has_pos else torch.zeros(src.shape[0], dtype=torch.float32, device=dev)
        _lib.call("as_mean_contour_fit", src, src_rel, rows, self.offsets, vocab_size, D, bank, rel, table)
        self.bank, self.table = bank, table
        self.rel_pos = rel if has_pos else None
        self.positions = src_pos[rows] if has_pos else None
        self.rows = rows if src_rows is None else src_rows[rows]
        self.sampled = bool(frac < 1.0)
        return self

    def fit(self, dataset, frac=0.1, random_state=0, device=None):
        """Tabulates ``dataset`` (8-field utterance items, or an ``HBMResidentDataset`` of them) and keeps the reference's per-token
        sample: the data set is uploaded once, the run positions come from ``as_token_runs``, the sample is drawn on the host and
        compacted on the device.  ``frac=1.0`` keeps every frame."""
        from ..encoder_decoder.dataset import HBMResidentDataset
        if not isinstance(dataset, HBMResidentDataset):
            device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            dataset = HBMResidentDataset(dataset, device)
        if self.articulators is None:
            self.articulators = list(dataset.articulators)
        if self.vocabulary is None and dataset.vocabulary is not None:
            self.vocabulary = dict(dataset.vocabulary)
        targets = dataset._targets
        if targets.dim() != 4 or targets.shape[1] != len(self.articulators) or targets.shape[2] != 2:
            raise ValueError(f"targets {tuple(targets.shape)}: expected (frames, {len(self.articulators)}, 2, n_samples)")
        self.n_samples = int(targets.shape[3])
        tokens_host = dataset._tokens.cpu().numpy()
        vocab_size = len(self.vocabulary) if self.vocabulary else int(tokens_host.max()) + 1
        if tokens_host.size and (tokens_host.min() < 0 or tokens_host.max() >= vocab_size):
            raise ValueError(f"the data set holds token ids outside [0, {vocab_size})")
        abs_pos, seq_len, rel_pos = token_runs(dataset._tokens, dataset._first, [m[3] for m in dataset._meta])
        return self._build(targets, rel_pos, torch.stack([abs_pos, seq_len], dim=1), None, tokens_host, vocab_size, frac, random_state)

    def _bank_tokens(self):
        return np.repeat(np.arange(self.vocab_size), np.diff(self._offsets_host))

    def resample(self, frac=0.1, random_state=0):
        """A new model holding the reference's per-token sample of this model's bank (the ``.sample(frac=0.1, random_state=0)`` of
        :103 / :130 applied to a full table): what ``fit(dataset, frac)`` gives when this model is ``fit(dataset, 1.0)``."""
        self._require_fit()
        other = PhonemeWiseMeanContour(self.vocabulary, self.articulators, self.n_samples)
        return other._build(self.bank, self.rel_pos, self.positions, self.rows, self._bank_tokens(), self.vocab_size, frac, random_state)

    def _require_fit(self):
        if self.bank is None:
            raise RuntimeError("this PhonemeWiseMeanContour has not been fitted")

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, tokens, lengths, weighted=False):
        """tokens (B, T) integer ids on the device, lengths (B,) -> (B, T, A, 2, N) float32: the token's mean contour
        (``weighted=False``) or its position-weighted mean; zeros on padded frames (t >= length).  A valid frame whose token has no
        stored frame raises IndexError naming the tokens (lazily with ``defer_token_check``)."""
        self._require_fit()
        _lib.require_gpu(tokens, "tokens")
        if tokens.dim() != 2:
            raise ValueError(f"tokens {tuple(tokens.shape)}: expected (B, T)")
        if weighted and self.rel_pos is None:
            raise ValueError("this table holds no positions (abs_pos / seq_len / rel_pos): it was made for the unweighted method")
        dev = self.bank.device
        tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
        B, T = tokens.shape
        lens_host = torch.as_tensor(lengths, dtype=torch.int32, device="cpu") if not (torch.is_tensor(lengths) and lengths.is_cuda) else None
        if lens_host is not None:
            if lens_host.numel() != B or (B and (int(lens_host.min()) < 0 or int(lens_host.max()) > T)):
                raise ValueError(f"lengths must hold {B} values in [0, {T}]")
            lens = lens_host.to(dev, non_blocking=True)
        else:
            lens = lengths.to(dtype=torch.int32).contiguous()
        out = torch.empty((B, T, len(self.articulators), 2, self.n_samples), dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        V, D = self.vocab_size, self.row_elems
        if weighted:
            first = torch.arange(B, dtype=torch.int64) * T
            _, _, rel = token_runs(tokens.view(-1), first, lens_host if lens_host is not None else lens)
            _lib.call("as_mean_contour_weighted_fwd", self.bank, self.rel_pos, self.offsets, tokens, rel, lens, B, T, V, D, out, flag)
        else:
            _lib.call("as_mean_contour_fwd", self.table, self.offsets, tokens, lens, B, T, V, D, out, flag)
        self._pending.append((flag, tokens, lens))
        if not self.defer_token_check:
            self.check_tokens()
        return out

    __call__ = forward

    def check_tokens(self):
        pending, self._pending = self._pending, []
        for flag, tokens, lens in pending:
            if int(flag.item()):
                valid = torch.arange(tokens.shape[1], device=tokens.device)[None, :] < lens[:, None]
                require_bank(self._offsets_host, tokens[valid].cpu().numpy(), self.vocabulary)

    def numerize(self, sentence_tokens):
        """token strings -> ids of this model's vocabulary; a string outside it is an error naming it"""
        if self.vocabulary is None:
            raise RuntimeError("this model has no vocabulary")
        unknown = sorted({t for t in sentence_tokens if t not in self.vocabulary})
        if unknown:
            raise IndexError("phoneme-wise mean contour: no stored frame for token(s) " + ", ".join(repr(t) for t in unknown) +
                             " (not in the table's vocabulary)")
        return torch.tensor([self.vocabulary[t] for t in sentence_tokens], dtype=torch.int64)

    # ------------------------------------------------------------------------------------------------ persistence
    def state_dict(self):
        self._require_fit()
        sd = OrderedDict(bank=self.bank.clone(), offsets=self.offsets.clone(), table=self.table.clone(), rows=self.rows.clone())
        if self.rel_pos is not None:
            sd["rel_pos"], sd["positions"] = self.rel_pos.clone(), self.positions.clone()
        sd["articulators"], sd["vocabulary"], sd["sampled"] = list(self.articulators), dict(self.vocabulary or {}), self.sampled
        return sd

    def load_state_dict(self, state_dict, device=None):
        missing = {"bank", "offsets", "table", "rows", "articulators", "vocabulary"} - set(state_dict)
        if missing:
            raise RuntimeError(f"Missing key(s) in state_dict: {sorted(missing)}")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        bank, offsets = state_dict["bank"], state_dict["offsets"]
        if bank.dim() != 4 or bank.shape[1] != len(state_dict["articulators"]) or bank.shape[2] != 2:
            raise RuntimeError(f"size mismatch for bank: {tuple(bank.shape)}")
        offsets_host = offsets.cpu().numpy().astype(np.int64)
        if offsets_host[0] != 0 or (np.diff(offsets_host) < 0).any() or offsets_host[-1] != bank.shape[0]:
            raise RuntimeError("offsets do not describe the bank")
        if tuple(state_dict["table"].shape) != (len(offsets_host) - 1, *bank.shape[1:]):
            raise RuntimeError(f"size mismatch for table: {tuple(state_dict['table'].shape)}")
        self.articulators, self.vocabulary = list(state_dict["articulators"]), dict(state_dict["vocabulary"]) or None
        self.n_samples, self.sampled = int(bank.shape[3]), bool(state_dict.get("sampled", False))
        self.bank, self.table = bank.to(dev, torch.float32).contiguous(), state_dict["table"].to(dev, torch.float32).contiguous()
        self.offsets, self._offsets_host = offsets.to(dev, torch.int64).contiguous(), offsets_host
        self.rows = state_dict["rows"].to(dev, torch.int64)
        self.rel_pos = state_dict["rel_pos"].to(dev, torch.float32).contiguous() if "rel_pos" in state_dict else None
        self.positions = state_dict["positions"].to(dev, torch.int32) if "positions" in state_dict else None
        return self

    def to_csv(self, path, positions=None):
        """The reference's table file (``pd.DataFrame(data).to_csv(index=False)``, :155-157): ``token[, abs_pos, seq_len, rel_pos]``
        and one stringified ``[[x...], [y...]]`` list per articulator, rows in table order.  ``positions``: write the three position
        columns (default: when the model holds them; ``train`` follows its ``weighted``).  A table file is read back as a FULL table
        (the sample is drawn at load time), so a sampled model is refused."""
        self._require_fit()
        if self.sampled:
            raise ValueError("to_csv writes the full table; this model holds a sample of it (fit with frac=1.0, or keep its state_dict)")
        positions = self.rel_pos is not None if positions is None else bool(positions)
        if positions and self.rel_pos is None:
            raise ValueError("this table holds no positions")
        names = {i: t for t, i in self.vocabulary.items()}
        order = torch.argsort(self.rows).cpu().numpy()
        tokens = [names[int(v)] for v in self._bank_tokens()[order]]
        return write_table(path, tokens, self.positions.cpu().numpy()[order] if positions else None, self.bank.cpu().numpy()[order],
                           self.articulators)

    @classmethod
    def from_csv(cls, path, vocabulary=None, device=None):
        """Reads a table file written by the reference's ``train`` (or by ``to_csv``) as a full table; ``resample`` then draws the
        forward pass's sample.  Tokens missing from ``vocabulary`` are appended to it in order of appearance."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        data = read_table(path)
        vocabulary = dict(vocabulary) if vocabulary else {}
        for token in data["tokens"]:
            if token not in vocabulary:
                vocabulary[token] = max(vocabulary.values(), default=-1) + 1
        tokens = np.array([vocabulary[t] for t in data["tokens"]], np.int64)
        model = cls(vocabulary, data["articulators"], data["contours"].shape[3])
        src_pos = src_rel = None
        if data["positions"] is not None:
            src_pos = torch.from_numpy(data["positions"]).to(dev, torch.int32)
            src_rel = src_pos[:, 0].float() / src_pos[:, 1].float()
        return model._build(torch.from_numpy(data["contours"]).to(dev), src_rel, src_pos, None, tokens, max(vocabulary.values()) + 1, 1.0, 0)


# ---------------------------------------------------------------------------------------------------- the reference's functions
def _as_model(df, device=None):
    if isinstance(df, PhonemeWiseMeanContour):
        return df
    if isinstance(df, (str, os.PathLike)):
        path = os.fspath(df)
        if path.endswith((".pt", ".pth")):
            return PhonemeWiseMeanContour().load_state_dict(torch.load(path, map_location="cpu"), device)
        return PhonemeWiseMeanContour.from_csv(path, device=device)
    raise TypeError(f"expected a PhonemeWiseMeanContour, a table file or a saved state_dict, got {type(df).__name__}")


def _forward_sentence(sentence_tokens, model, articulators, n_samples, weighted):
    if n_samples != model.n_samples:
        raise ValueError(f"n_samples={n_samples}, the table holds contours of {model.n_samples} points")
    tokens = model.numerize(sentence_tokens).to(model.bank.device)[None]
    out = model.forward(tokens, [tokens.shape[1]], weighted=weighted)[0]
    if list(articulators) != list(model.articulators):
        out = out[:, [model.articulators.index(a) for a in articulators]]
    return out


def forward_mean_contour(sentence_tokens, model, articulators, n_samples=50):
    """One sentence's token strings -> (len, n_articulators, 2, n_samples) on the device (reference :125-145)."""
    return _forward_sentence(sentence_tokens, model, articulators, n_samples, False)


def forward_weighted_mean_contour(sentence_tokens, model, articulators, n_samples=50):
    """One sentence's token strings -> (len, n_articulators, 2, n_samples) on the device (reference :86-122; float32 where the
    reference's softmin weights make it float64)."""
    return _forward_sentence(sentence_tokens, model, articulators, n_samples, True)


def train(dataset, save_to=None, weighted=False, frac=1.0, random_state=0, device=None):
    """The reference's ``train`` (:148-159) tabulates every training frame; so does this, on the device, and returns the model in
    place of the DataFrame.  ``save_to``: the table file, with the position columns when ``weighted`` (``process_sentence_with_pos``
    against ``process_sentence``).  The forward pass's sample is drawn by ``test`` (or ``resample``), as in the reference; ``frac`` < 1
    keeps only a sample here (such a model has no table file)."""
    vocabulary = getattr(dataset, "vocabulary", None)
    model = PhonemeWiseMeanContour(vocabulary, getattr(dataset, "articulators", None)).fit(dataset, frac, random_state, device)
    if save_to is not None:
        model.to_csv(save_to, positions=weighted)
    return model


def test(dataset, df, save_to, weighted=False, frac=0.1, random_state=0, batch_size=32, regularize_out=False, device=None,
         report_dir=None):
    """The reference's ``test`` (:162-254): ``df`` is a model, a table file or a saved state_dict; a full table is first reduced to
    the reference's per-token sample (``frac``, ``random_state``; ``frac=None`` keeps the bank as it is).  Per sentence: the mean
    Euclidean distance, the Pearson correlations, tract variables and contour dumps under ``save_to/0`` with the upper incisor
    injected from the reference contour; sentences are evaluated ``batch_size`` at a time, one launch per batch.  Returns
    ``{"loss", articulator: {"x_corr", "y_corr"}}``, each the mean over sentences.  ``regularize_out`` (the reference passes True)
    needs the external vt_tools package.  ``report_dir``: also write the result tables of ..report there, from the frames of this
    pass."""
    from ..encoder_decoder.evaluation import _Accumulator
    from ..metrics import EuclideanDistance
    model = _as_model(df, device)
    if frac is not None and frac < 1.0 and not model.sampled:
        model = model.resample(frac, random_state)
    dev = model.bank.device
    articulators = list(dataset.articulators)
    channels = None if articulators == list(model.articulators) else [model.articulators.index(a) for a in articulators]
    save_to = os.path.join(save_to, "0")  # Keep compatibility with other methods
    os.makedirs(save_to, exist_ok=True)
    criterion = EuclideanDistance()
    acc = _Accumulator(articulators, save_to, dev, regularize_out, report_dir, getattr(dataset, "dataset_config", None))
    for start in range(0, len(dataset), batch_size):
        items = [dataset[i] for i in range(start, min(start + batch_size, len(dataset)))]
        lengths = [len(item[3]) for item in items]
        tokens = torch.nn.utils.rnn.pad_sequence([model.numerize(item[3]) for item in items], batch_first=True).to(dev)
        with torch.no_grad():
            outputs = model.forward(tokens, lengths, weighted=weighted)
        if channels is not None:
            outputs = outputs[:, :, channels]
        for b, (item, length) in enumerate(zip(items, lengths)):
            sentence_name, _, sentence_targets, sentence_tokens, reference_arrays, _, frame_ids, _ = item
            sentence_outputs = outputs[b:b + 1, :length].contiguous()
            sentence_targets = sentence_targets.float().to(dev).unsqueeze(dim=0)
            loss = criterion(sentence_outputs, sentence_targets)
            acc.add(loss.item(), sentence_outputs, sentence_targets, [length], [sentence_name], [frame_ids], [sentence_tokens],
                    reference_arrays.float().unsqueeze(dim=0))
    acc.write_report()
    info = {"loss": float(np.mean(acc.losses))}
    info.update({
        art: {"x_corr": float(np.mean(acc.x_corrs[i])), "y_corr": float(np.mean(acc.y_corrs[i]))}
        for i, art in enumerate(articulators)
    })
    return info


# ---------------------------------------------------------------------------------------------------- synthetic data
class SyntheticSegmentedArtSpeechDataset(Dataset):
    """Seeded synthetic utterances with phoneme RUNS, in the 8-field layout of ``ArtSpeechDataset.__getitem__``.

    An utterance of ``min_len`` .. ``max_len`` frames is a sequence of runs: a token in [2, V) (0 = <blank> the pad id, 1 = <unk>;
    never the previous run's token; token v drawn with weight exp(-token_skew * (v - 2)), so the last tokens can be made rare) held
    for 1 .. ``max_duration`` frames.  A frame's contour is the token's own shape plus a smooth trajectory in the frame's relative
    position inside its run plus noise:  shape[v] + amplitude * sin(pi * (rel_pos - 1/2)) * direction[v] + noise * N(0, 1),
    so a method that knows the position (the weighted mean contour) is measurably better than one that does not."""

    def __init__(self, num_sentences, vocabulary, articulators, n_samples=50, min_len=20, max_len=200, max_duration=30, seed=0,
                 database_name="artspeech2", voiced_tokens=None, token_skew=0.0, amplitude=0.3, noise=0.02):
        self.vocabulary = vocabulary
        self.articulators = sorted(articulators)
        self.num_articulators = len(articulators)
        self.num_samples = n_samples
        self.dataset_config = DATASET_CONFIG[database_name]
        self.voiced_tokens = voiced_tokens or []
        self.max_duration, self.amplitude, self.noise = int(max_duration), float(amplitude), float(noise)
        self._tokens_by_id = {i: t for t, i in vocabulary.items()}
        V = len(vocabulary)
        if V < 4:
            raise ValueError("the vocabulary must hold at least two tokens besides <blank> and <unk>")
        # the shapes belong to the vocabulary, not to the split: every split of one (vocabulary size, articulators, n_samples)
        # shares them, whatever its seed
        shapes = torch.Generator().manual_seed(1234567)
        self._shape = 0.25 + 0.5 * torch.rand(V, self.num_articulators, 2, n_samples, generator=shapes)
        self._direction = torch.rand(V, self.num_articulators, 2, n_samples, generator=shapes) - 0.5
        self._weights = torch.exp(-float(token_skew) * torch.arange(V - 2, dtype=torch.float64))
        g = torch.Generator().manual_seed(seed)
        self._lengths = torch.randint(min_len, max_len + 1, (num_sentences,), generator=g).tolist()
        self._seeds = torch.randint(0, 2 ** 31 - 1, (num_sentences,), generator=g).tolist()

    def __len__(self):
        return len(self._lengths)

    def __getitem__(self, index):
        length = self._lengths[index]
        g = torch.Generator().manual_seed(self._seeds[index])
        ids, rel, previous = [], [], -1
        while len(ids) < length:
            weights = self._weights.clone()
            if previous >= 0:
                weights[previous - 2] = 0.0
            token = int(torch.multinomial(weights, 1, generator=g)) + 2
            duration = min(int(torch.randint(1, self.max_duration + 1, (1,), generator=g)), length - len(ids))
            ids += [token] * duration
            rel += [i / duration for i in range(duration)]
            previous = token
        sentence_numerized = torch.tensor(ids, dtype=torch.long)
        swing = torch.sin(np.pi * (torch.tensor(rel, dtype=torch.float32) - 0.5)).view(length, 1, 1, 1)
        sentence_targets = (self._shape[sentence_numerized] + self.amplitude * swing * self._direction[sentence_numerized]
                            + self.noise * torch.randn(length, self.num_articulators, 2, self.num_samples, generator=g))
        reference_arrays = torch.rand(length, 1, 2, self.num_samples, generator=g)
        sentence_tokens = [self._tokens_by_id.get(int(i), UNKNOWN) for i in sentence_numerized]
        voicing = torch.tensor([t in self.voiced_tokens for t in sentence_tokens], dtype=torch.float)
        critical_masks = torch.tensor([], dtype=torch.int)
        frame_ids = [f"{i:04d}" for i in range(length)]
        return (f"synthetic_{index:05d}", sentence_numerized, sentence_targets, sentence_tokens, reference_arrays,
                critical_masks, frame_ids, voicing)
