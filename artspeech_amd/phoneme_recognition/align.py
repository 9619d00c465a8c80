"""The recogniser's evaluation kernels (csrc/recog_eval.hip) as checked wrappers: device tensors in, device tensors out, nothing
copied to the host.

* ``decode_top1``      -- arg-max per frame, repeats collapsed, blank dropped (reference decoders.py:36-42).
* ``edit_distance``    -- Levenshtein distance of padded token batches (torchmetrics' word_error_rate distance, metrics.py:135).
* ``align_counts``     -- substitution / insertion / deletion counts along the reference's alignment path (metrics.py:295-381).
* ``confusion_counts`` -- frame-level (target class, predicted class) counts (``compute_confusion_matrix``, __init__.py:410-432).

Token batches are (B, pitch) integer tensors with a count per row; ``class_map`` (one class per token id) is applied to both
sides before comparing, which is how the reference aligns phonetic groups instead of phonemes."""

import torch

from .. import _lib
from . import emission_args as args
from .emission_args import MAX_TARGET   # as_edit_distance / as_align_counts: the CTC kernels' limit

MAX_FRAMES = 8192   # as_decode_top1
MAX_PRED = 4096     # as_edit_distance / as_align_counts


def _i32(t, dev):
    return torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous()


def _counts(v, B, dev, what):
    t = torch.as_tensor(v).reshape(-1)
    if t.numel() != B:
        raise ValueError(f"{what} must have one entry per utterance ({B}), got {t.numel()}")
    return t.to(device=dev, dtype=torch.int32).contiguous()   # a strided view (one column of a (B, n) tensor) becomes dense


def _ptr(t):
    return t if t is not None and t.numel() else None   # an empty tensor goes as NULL


def _class_map(class_map, dev):
    if class_map is None:
        return None, 0
    m = _i32(class_map, dev).reshape(-1)
    if m.numel() == 0:
        raise ValueError("class_map must have at least one entry")
    return m, m.numel()


def decode_top1(emissions, lengths=None, blank=-1, return_argmax=False):
    """emissions (B, T, C) float32 in any batch and time strides -> (tokens (B, T) int32 padded with -1, counts (B,) int32) and,
    with return_argmax, the raw per-frame arg-max (B, T) int32 (-1 past the length).  lengths: one entry per utterance, or None
    for all T frames; blank < 0 or None: no blank token."""
    _lib.require_gpu(emissions, "emissions")
    emissions, T, B, Cn, st, sb = args.emissions(emissions, "decode_top1", False, detach=True)
    dev = emissions.device
    if T > MAX_FRAMES:
        raise ValueError(f"decode_top1: {T} frames exceeds the supported {MAX_FRAMES}")
    tokens = torch.empty(B, T, device=dev, dtype=torch.int32)
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    argmax = torch.empty(B, T, device=dev, dtype=torch.int32) if return_argmax else None
    if lengths is not None:
        _, lengths = args.lengths(lengths, B, "decode_top1", device=dev)
    if B and T and Cn:
        _lib.call("as_decode_top1", emissions, sb, st, B, T, Cn, lengths,
                  -1 if blank is None else int(blank), tokens, counts, argmax)
    else:
        tokens.fill_(-1)
        counts.zero_()
        if argmax is not None:
            argmax.fill_(-1)
    return (tokens, counts, argmax) if return_argmax else (tokens, counts)


def _pairs(who, pred, pred_counts, target, target_counts):
    _lib.require_gpu(pred, "pred")
    dev = pred.device
    if pred.dim() != 2 or torch.as_tensor(target).dim() != 2:
        raise ValueError(f"{who}: pred and target must be (B, pitch) token batches")
    target = _i32(target, dev)
    pred = _i32(pred, dev)
    B = pred.shape[0]
    if target.shape[0] != B:
        raise ValueError(f"{who}: {B} predictions but {target.shape[0]} targets")
    pc, tc = _counts(pred_counts, B, dev, f"{who}: pred_counts"), _counts(target_counts, B, dev, f"{who}: target_counts")
    if pred.shape[1] > MAX_PRED or target.shape[1] > MAX_TARGET:
        raise ValueError(f"{who}: {pred.shape[1]} predicted / {target.shape[1]} target tokens exceeds the supported "
                         f"{MAX_PRED} / {MAX_TARGET}")
    return pred, pc, target, tc, B, dev


def edit_distance(pred, pred_counts, target, target_counts, class_map=None):
    """Levenshtein distance (insertions, deletions, substitutions cost 1) of every (prediction, target) pair -> (B,) int32."""
    pred, pc, target, tc, B, dev = _pairs("edit_distance", pred, pred_counts, target, target_counts)
    cm, n_map = _class_map(class_map, dev)
    dist = torch.empty(B, device=dev, dtype=torch.int32)
    if B:
        _lib.call("as_edit_distance", _ptr(pred), pred.shape[1], pc, _ptr(target), target.shape[1], tc, B, cm, n_map, dist)
    return dist


def align_counts(pred, pred_counts, target, target_counts, n_classes, class_map=None, out=None):
    """Adds the alignment counts of every pair into ``out`` ((n_classes + 1, n_classes + 1) int32, created zeroed when None):
    out[target class, predicted class] for diagonal moves (matches included), out[target class, n_classes] for deletions,
    out[n_classes, predicted class] for insertions.  Returns (out, distances (B,) int32)."""
    pred, pc, target, tc, B, dev = _pairs("align_counts", pred, pred_counts, target, target_counts)
    cm, n_map = _class_map(class_map, dev)
    n_classes = int(n_classes)
    if n_classes <= 0:
        raise ValueError("align_counts: n_classes must be positive")
    if out is None:
        out = torch.zeros(n_classes + 1, n_classes + 1, device=dev, dtype=torch.int32)
    else:
        _lib.require_gpu(out, "out")
        if out.shape != (n_classes + 1, n_classes + 1) or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError(f"align_counts: out must be a contiguous int32 ({n_classes + 1}, {n_classes + 1}) matrix")
    dist = torch.empty(B, device=dev, dtype=torch.int32)
    if B:
        nbytes = int(_lib.call("as_align_workspace_bytes", B, pred.shape[1], target.shape[1]))
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        _lib.call("as_align_counts", _ptr(pred), pred.shape[1], pc, _ptr(target), target.shape[1], tc, B, cm, n_map, n_classes, out, dist,
                  ws, nbytes)
    return out, dist


def confusion_counts(argmax, targets, lengths, n, class_map=None, out=None):
    """Adds 1 to out[class(targets[b, t]), class(argmax[b, t])] for every frame t < min(lengths[b], T, S) (lengths None: all) ->
    out (n, n) int32, created zeroed when None.  argmax (B, T), targets (B, S); frames of class outside [0, n), such as the -1
    padding, are skipped."""
    _lib.require_gpu(argmax, "argmax")
    dev = argmax.device
    if argmax.dim() != 2 or torch.as_tensor(targets).dim() != 2:
        raise ValueError("confusion_counts: argmax and targets must be (B, T) and (B, S)")
    argmax, targets = _i32(argmax, dev), _i32(targets, dev)
    B = argmax.shape[0]
    if targets.shape[0] != B:
        raise ValueError(f"confusion_counts: {B} predictions but {targets.shape[0]} targets")
    n = int(n)
    if n <= 0:
        raise ValueError("confusion_counts: n must be positive")
    if lengths is not None:
        _, lengths = args.lengths(lengths, B, "confusion_counts", device=dev)
    cm, n_map = _class_map(class_map, dev)
    if out is None:
        out = torch.zeros(n, n, device=dev, dtype=torch.int32)
    else:
        _lib.require_gpu(out, "out")
        if out.shape != (n, n) or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError(f"confusion_counts: out must be a contiguous int32 ({n}, {n}) matrix")
    if B and argmax.shape[1] and targets.shape[1]:
        _lib.call("as_confusion_counts", argmax, argmax.shape[1], targets, targets.shape[1], lengths, B, cm, n_map, n, out)
    return out
