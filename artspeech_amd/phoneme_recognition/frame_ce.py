"""Frame-level cross-entropy on the HIP library (as_frame_ce_loss / as_frame_ce_grad) and the rank statistic of the AUROC
(as_frame_auroc): the device side of the reference's ``loss: CE`` criterion, ``CrossEntropyLoss.forward`` (phoneme_recognition/
metrics.py:110-120) -- ``nn.CrossEntropyLoss`` over the emission frames and target entries that the pad masks keep.

``frame_cross_entropy(x, ...)`` takes the (T, B, C) rows in any strides whose class stride is 1 -- the permuted view of a
(B, T, C) tensor costs no copy -- and padded (B, S) targets, one per frame.  The reference pairs the flattened valid frames with
the flattened valid target entries, which pairs frame t with target t only when the two length vectors are equal: they must be.
Weights, ``ignore_index`` and ``label_smoothing`` follow ``torch.nn.functional.cross_entropy``; reductions are ``mean`` (the sum
of the frame losses over the sum of their target weights; NaN without a valid frame) and ``sum``.  The loss, the division and the
backward's scale stay on the device: nothing synchronises."""
import torch

from .. import _lib
from . import emission_args as args

MAX_CLASSES = 4096        # as_frame_ce_loss
MAX_AUROC_FRAMES = 16384  # as_frame_auroc sorts a class column in LDS

_tickets = {}   # (device, stream) -> the loss kernel's workspace: its ticket starts at zero and every call leaves it there


def _workspace(dev, nbytes):
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _tickets.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _tickets[key] = torch.zeros(max(nbytes, 8 + 16 * 256), device=dev, dtype=torch.uint8)
    return ws


def check_frame_lengths(who, input_lengths, target_lengths, B, T):
    """The two length vectors as one host int64 (B,) tensor; ValueError unless they are equal entry by entry and lie in [0, T]."""
    il, _ = args.lengths(input_lengths, B, who, "input_lengths", host=True)
    tl, _ = args.lengths(target_lengths, B, who, "target_lengths", host=True)
    differ = (il != tl).nonzero()
    if differ.numel():
        b = int(differ[0])
        raise ValueError(f"{who}: one target per frame is required, but utterance {b} has {int(il[b])} frames and {int(tl[b])} "
                         f"target entries")
    return args.lengths(il, B, who, T=T)[0]


def _frame_targets(who, targets, B, T, dev):
    targets = torch.as_tensor(targets)
    if targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError(f"{who}: targets must be padded (B, S) rows, one entry per frame")
    return targets.to(device=dev, dtype=torch.int64).contiguous()


class _FrameCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, st, sb, targets, lengths, weight, ignore_index, mean, label_smoothing):
        T, B, Cn = x.shape
        dev = x.device
        lse = torch.empty(B, T, device=dev, dtype=torch.float32)
        sums = torch.empty(2, device=dev, dtype=torch.float64)
        nbytes = int(_lib.call("as_frame_ce_workspace_bytes", T, B))
        ws = _workspace(dev, nbytes)
        _lib.call("as_frame_ce_loss", x, st, sb, T, B, Cn, targets, targets.shape[1], lengths, weight, ignore_index,
                  label_smoothing, lse, sums, ws, ws.numel())
        out = (sums[0] / sums[1] if mean else sums[0]).to(torch.float32)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, targets, lengths, lse, sums, *([weight] if weight is not None else []))
            ctx.meta = (ignore_index, mean, label_smoothing, st, sb)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, targets, lengths, lse, sums, *weight = ctx.saved_tensors
        ignore_index, mean, label_smoothing, st, sb = ctx.meta
        T, B, Cn = x.shape
        gout = gout.to(torch.float32).reshape(1).contiguous()
        grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        _lib.call("as_frame_ce_grad", x, st, sb, T, B, Cn, targets, targets.shape[1], lengths,
                  weight[0] if weight else None, ignore_index, label_smoothing, lse, sums, gout, int(mean), grad, grad.stride(0),
                  grad.stride(1))
        return grad, None, None, None, None, None, None, None, None


def frame_cross_entropy(x, targets, input_lengths, target_lengths, weight=None, ignore_index=-100, reduction="mean",
                        label_smoothing=0.0):
    """``torch.nn.functional.cross_entropy`` over the frames t < input_lengths[b] of x (T, B, C) against targets[b, t], on the HIP
    library (see the module docstring).  ``input_lengths[b] == target_lengths[b]`` for every b, else ValueError."""
    if reduction == "none":
        raise NotImplementedError("frame_cross_entropy: reduction='none' is not built (the reference never asks for it); "
                                  "use 'mean' or 'sum'")
    if reduction not in ("sum", "mean"):
        raise ValueError(f"frame_cross_entropy: unknown reduction {reduction!r}")
    T, B, Cn = args.emissions_shape(x, "frame_cross_entropy", True, "x")
    il = check_frame_lengths("frame_cross_entropy", input_lengths, target_lengths, B, T)
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError(f"frame_cross_entropy: label_smoothing {label_smoothing} outside [0, 1]")
    _lib.require_gpu(x, "x")
    x, T, B, Cn, st, sb = args.emissions(x, "frame_cross_entropy", True, name="x")
    if not 1 <= Cn <= MAX_CLASSES:
        raise ValueError(f"frame_cross_entropy (HIP): {Cn} classes outside the supported 1..{MAX_CLASSES}")
    dev = x.device
    targets = _frame_targets("frame_cross_entropy", targets, B, T, dev)
    if B and targets.shape[1] < int(il.max()):
        raise ValueError("frame_cross_entropy: padded targets must be (B, S) with S >= max(lengths)")
    if weight is not None:
        weight = torch.as_tensor(weight).to(device=dev, dtype=torch.float32).contiguous()
        if weight.shape != (Cn,):
            raise ValueError(f"frame_cross_entropy: weight must have one entry per class ({Cn}), got {tuple(weight.shape)}")
    if B == 0 or T == 0:
        zero = x.sum() * 0.0
        return zero / zero if reduction == "mean" else zero
    if targets.shape[1] < T:   # the kernel reads targets[b, t] for t < lengths[b] <= S only, but takes one pitch >= T
        targets = torch.nn.functional.pad(targets, (0, T - targets.shape[1]), value=int(ignore_index))
    return _FrameCE.apply(x, st, sb, targets, il.to(dev), weight, int(ignore_index), reduction == "mean", float(label_smoothing))


def frame_auroc_counts(scores, targets, lengths, ignore_index=-100):
    """(n_pos, n_neg, u2), int64 (C,) on the device: per class c the one-vs-rest rank statistic of scores[b, t, c] (B, T, C; ranked
    as given) over the frames t < lengths[b] whose target lies in [0, C) and is not ignore_index -- the number of positive and
    negative frames and twice the number of (positive, negative) pairs the positive outranks, ties counted once.
    AUROC_c = u2 / (2 n_pos n_neg).  At most MAX_AUROC_FRAMES frames (ValueError beyond: there is no workspace path)."""
    _lib.require_gpu(scores, "scores")
    scores, T, B, Cn, st, sb = args.emissions(scores, "frame_auroc_counts", False, detach=True, name="scores")
    dev = scores.device
    targets = _frame_targets("frame_auroc_counts", targets, B, T, dev)
    lengths, lengths_dev = args.lengths(lengths, B, "frame_auroc_counts", device=dev)
    out = torch.zeros(3, max(Cn, 1), device=dev, dtype=torch.int64)
    if B == 0 or T == 0 or Cn == 0:
        return out[0, :Cn], out[1, :Cn], out[2, :Cn]
    # the bound on the number of frames: from the lengths when they are on the host (no synchronisation either way)
    frames = B * T if lengths.is_cuda else int(lengths.clamp(0, min(T, targets.shape[1])).sum())
    if frames > MAX_AUROC_FRAMES:
        raise ValueError(f"frame_auroc_counts: {frames} frames exceeds the supported {MAX_AUROC_FRAMES}")
    if targets.shape[1] < T:
        targets = torch.nn.functional.pad(targets, (0, T - targets.shape[1]), value=int(ignore_index))
    _lib.call("as_frame_auroc", scores, st, sb, T, B, Cn, targets, targets.shape[1], lengths_dev,
              int(ignore_index), max(frames, 1), out[0], out[1], out[2])
    return out[0], out[1], out[2]
