"""phoneme_to_articulation package of the MI355X engine (reference: phoneme_to_articulation/__init__.py)."""
import csv
import os
from enum import Enum

import numpy as np
import torch.nn as nn


class RNNType(Enum):
    """Recurrent cell switch (reference phoneme_to_articulation/__init__.py:47-49).  The values are the torch classes only
    because the reference's are (they serve as PARAMETER CONTAINERS here: same keys, shapes and initialisation); the
    recurrences run on the HIP kernels of csrc/gru.hip and csrc/lstm.hip."""
    LSTM = nn.LSTM
    GRU = nn.GRU


def save_outputs(sentences_ids, frame_ids, outputs, targets, lengths, phonemes, articulators, save_to, regularize_out=False):
    """Per-sentence contour dumps of the test loops (reference phoneme_to_articulation/__init__.py:121-198): for every valid
    frame and articulator (sorted names) ``<save_to>/<sentence>/contours/<frame>_<articulator>.npy`` (prediction, (2, N)
    float32) and ``..._true.npy`` (target), plus ``phonemes.csv`` (sentence, frame, phoneme).  ``outputs`` / ``targets``
    (bs, seq_len, n_articulators, 2, n_samples) are copied to the host once per batch.  ``regularize_out`` asks for the
    B-spline regularisation of the un-vendored ``vt_tools`` package (:178-180), which this build does not restate."""
    if regularize_out:
        raise NotImplementedError("regularize_out=True needs vt_tools.bs_regularization.regularize_Bsplines (external package)")
    outputs = outputs.detach().cpu().numpy() if hasattr(outputs, "detach") else np.asarray(outputs)
    targets = targets.detach().cpu().numpy() if hasattr(targets, "detach") else np.asarray(targets)
    names = sorted(articulators)
    for b, (sentence_id, length) in enumerate(zip(sentences_ids, lengths)):
        contour_dir = os.path.join(save_to, sentence_id, "contours")
        os.makedirs(contour_dir, exist_ok=True)
        rows = []
        for t, (phoneme, frame) in enumerate(zip(phonemes[b], frame_ids[b])):
            if t >= int(length):
                break
            rows.append((sentence_id, frame, phoneme))
            for i_art, art in enumerate(names):
                np.save(os.path.join(contour_dir, f"{frame}_{art}.npy"), outputs[b, t, i_art])
                np.save(os.path.join(contour_dir, f"{frame}_{art}_true.npy"), targets[b, t, i_art])
        with open(os.path.join(save_to, sentence_id, "phonemes.csv"), "w", newline="") as f:
            writer = csv.writer(f, lineterminator="\n")  # pandas.DataFrame.to_csv(index=False) layout
            writer.writerow(("sentence", "frame", "phoneme"))
            writer.writerows(rows)


REQUIRED_ARTICULATORS_FOR_TVS = ["lower-lip", "pharynx", "soft-palate-midline", "tongue", "upper-lip", "upper-incisor"]  # :25-32


def tract_variables(sentences_ids, frame_ids, outputs, targets, lengths, phonemes, articulators, save_to):
    """``<save_to>/<sentence>/tract_variables.csv`` with the reference's columns (phoneme_to_articulation/__init__.py:
    201-297); the tract variables of all frames of the batch come from one launch of the HIP kernel."""
    from .encoder_decoder.evaluation import _write_tract_variables
    return _write_tract_variables(save_to, sentences_ids, frame_ids, outputs, targets, lengths, phonemes, articulators)


# ---- contour preparation (reference :52-118, tail_clipper.py, scripts/calculate_normalization_statistics.py) on the device:
# csrc/contours.hip.  Everything below is an addition; nothing above depends on it.
import torch  # noqa: E402
from functools import lru_cache  # noqa: E402

from .. import _lib  # noqa: E402
from ..settings import ArtSpeechConfig  # noqa: E402
from .tail_clipper import (  # noqa: E402,F401
    UPPER_INCISOR, TailClipper, clip_kinds, launch_prepare_contours, raise_on_empty)
from .transforms import Normalize  # noqa: E402


def load_articulator_array(filepath, norm_value):
    """One contour file as an (N, 2) float64 array divided by ``norm_value``.  The original is
    ``vt_shape_gen.helpers.load_articulator_array`` of an un-vendored, un-pinned package; this restatement is an ASSUMPTION
    (``np.load``, transposed to (N, 2) when the first dimension is 2, divided in float64) and its parity is unpinned, as
    SURVEY 8c says of ``vt_tools.metrics``."""
    array = np.asarray(np.load(filepath), dtype=np.float64)
    if array.ndim == 2 and array.shape[0] == 2:
        array = array.T
    return array / norm_value


@lru_cache(maxsize=None)
def cached_load_articulator_array(filepath, norm_value):
    """(N, 2) float32 tensor of a contour file (reference :52-54); only the file read is cached."""
    return torch.from_numpy(load_articulator_array(filepath, norm_value)).type(torch.float)


def _contour_path(datadir, subject, sequence, frame_id, articulator):
    return os.path.join(datadir, subject, sequence, "inference_contours", f"{frame_id}_{articulator}.npy")


def load_raw_contours(datadir, subject, sequence, frame_ids, articulators, norm_value=ArtSpeechConfig.RES):
    """The raw contours of one sequence's frames from ``<datadir>/<subject>/<sequence>/inference_contours/<frame>_<articulator>
    .npy``: raw (F, A, N, 2) and refs (F, 3, N, 2) (TailClipper.TAIL_CLIP_REFERENCES) float32 host tensors, the inputs of
    ``prepare_contours``.  ``norm_value`` is the data set's RES (136 for every database of settings.py)."""
    def stack(names):
        return torch.stack([torch.stack([cached_load_articulator_array(_contour_path(datadir, subject, sequence, frame_id, name),
                                                                       norm_value) for name in names]) for frame_id in frame_ids])
    return stack(articulators), stack(TailClipper.TAIL_CLIP_REFERENCES)


def prepare_contours(raw, refs, articulators, dataset_config, normalize=None, clip_tails=True, check=True):
    """Model targets from raw contours, all frames in one launch (as_prepare_contours): tails clipped (``clip_tails``), moved
    into the upper-incisor frame, normalised by ``normalize`` = {articulator: Normalize} (the dict the principal-components
    datasets carry) when given.  raw (F, A, N, 2), refs (F, 3, N, 2) on the GPU, any strides -> targets (F, A, 2, N), references
    (F, 1, 2, N), counts int32 (F, A), each (f, a) equal to the reference's ``prepare_articulator_array`` bit for bit.  A contour
    that keeps no point (the reference raises) has count 0 and a NaN row: with ``check`` a RuntimeError names the first one
    (one synchronisation, at data-set build time); without, the NaN row stands.  Clipping needs N = 50."""
    articulators = list(articulators)
    mean = std = None
    if normalize is not None:
        mean = torch.stack([torch.as_tensor(normalize[a].mean) for a in articulators])
        std = torch.stack([torch.as_tensor(normalize[a].std) for a in articulators])
    targets, references, counts = launch_prepare_contours(raw, refs, clip_kinds(articulators, clip_tails), dataset_config, mean, std)
    if check:
        raise_on_empty(counts, articulators)
    return targets, references, counts


def contour_statistics(x):
    """mean and unbiased std over the leading dimension of x (rows, ...) float32 on the GPU, each shaped x.shape[1:]: the
    ``.mean(axis=0)`` / ``.std(axis=0)`` of the reference's statistics script, accumulated in fp64 and rounded once
    (as_column_mean_std); one row gives NaN std, like torch."""
    _lib.require_gpu(x, "x")
    if x.dim() < 1 or x.shape[0] < 1 or x[0].numel() < 1:
        raise ValueError(f"contour_statistics needs at least one row and one column, got {tuple(x.shape)}")
    rows, shape = x.shape[0], tuple(x.shape[1:])
    x2 = x.to(torch.float32).reshape(rows, -1).contiguous()
    cols = x2.shape[1]
    parts = -(-rows // _lib.COLUMN_STATS_PART_ROWS)
    ws = torch.empty(2 * parts * cols, dtype=torch.float64, device=x.device)
    mean = torch.empty(cols, dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    with torch.cuda.device(x.device):
        _lib.call("as_column_mean_std", x2, rows, cols, mean, std, ws, ws.numel())
    return mean.reshape(shape), std.reshape(shape)


class InputLoaderMixin:
    @staticmethod
    def prepare_articulator_array(datadir, subject, sequence, frame_id, articulator, dataset_config, normalize_fn=None,
                                  clip_tails=True):
        """One (frame, articulator) with the reference's signature and return pair (reference :57-118): (contour (2, N),
        upper-incisor contour (2, N)) host tensors in the incisor frame.  It reads the files the reference reads (the three
        clipping references only with ``clip_tails``) and computes on the GPU; a ``Normalize`` goes into the launch, any other
        callable is applied to the result.  A whole sentence or corpus goes through ``load_raw_contours`` + ``prepare_contours``
        instead: one launch, not one per call."""
        if not torch.cuda.is_available():
            raise RuntimeError("artspeech_amd prepares contours on an MI355X device; there is no CPU path")
        def load(name):
            return cached_load_articulator_array(_contour_path(datadir, subject, sequence, frame_id, name), norm_value=dataset_config.RES)
        array = load(articulator)
        if clip_tails:
            refs = torch.stack([load(name) for name in TailClipper.TAIL_CLIP_REFERENCES])
        else:
            incisor = load(UPPER_INCISOR)
            refs = torch.stack([torch.zeros_like(incisor), incisor, torch.zeros_like(incisor)])
        dev = torch.device("cuda", torch.cuda.current_device())
        fused = isinstance(normalize_fn, Normalize)
        mean = torch.as_tensor(normalize_fn.mean)[None] if fused else None
        std = torch.as_tensor(normalize_fn.std)[None] if fused else None
        out, ref_out, counts = launch_prepare_contours(array[None, None].to(dev), refs[None].to(dev),
                                                       clip_kinds([articulator], clip_tails), dataset_config, mean, std)
        raise_on_empty(counts, [articulator], [frame_id])
        articulator_array = out[0, 0].cpu()
        if normalize_fn is not None and not fused:
            articulator_array = normalize_fn(articulator_array)
        return articulator_array, ref_out[0, 0].cpu()


class SyntheticRawContours:
    """Seeded raw contours for the statistics script and the benchmarks (the MRI corpora are private): raw (F, A, 50, 2) and
    refs (F, 3, 50, 2) from U(0, 1), with the lower incisor's y in [0.3, 0.7] and the epiglottis' y in [0.2, 0.7], so that the
    clipper cuts most tongues and lower lips and empties none (checked on 512 seeded frames with the reference's clipper)."""

    def __init__(self, num_frames, articulators, seed=0, n_samples=50):
        self.articulators = list(articulators)
        g = torch.Generator().manual_seed(seed)
        self.raw = torch.rand(num_frames, len(self.articulators), n_samples, 2, generator=g)
        self.refs = torch.rand(num_frames, 3, n_samples, 2, generator=g)
        self.refs[:, 0, :, 1] = 0.3 + 0.4 * self.refs[:, 0, :, 1]
        self.refs[:, 2, :, 1] = 0.2 + 0.5 * self.refs[:, 2, :, 1]
        self.frame_names = [f"synthetic_S0_{i:06d}" for i in range(num_frames)]

    def __len__(self):
        return self.raw.shape[0]
