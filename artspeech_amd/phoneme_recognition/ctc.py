"""CTC loss on the HIP library (as_ctc_loss / as_ctc_grad): a drop-in for ``torch.nn.CTCLoss`` as the reference calls it,
``criterion(log_softmax(outputs).permute(1, 0, 2), targets, input_lengths, target_lengths)`` (phoneme_recognition/__init__.py:
112-120).

``ctc_loss(x, ...)`` takes the (T, B, C) rows in any strides whose class stride is 1 -- the permuted view of a (B, T, C) tensor
costs no copy -- and targets either padded (B, S) (the reference's collate pads them with -1) or torch's concatenated 1-D form.
``logits=False``: x holds log-probabilities (torch semantics); ``logits=True``: x holds raw scores and the kernel normalises them
itself, so a trainer can skip the log-softmax pass: the gradient is then taken with respect to the scores.  Reductions and
``zero_infinity`` follow torch: ``mean`` divides each utterance's loss by max(target_length, 1), then averages over the batch.
"""
import ctypes as C

import torch

from .. import _lib

_MAX_TARGET = 2047  # S = 2L + 1 <= 4095 states (as_ctc_loss)


def _lengths(v, B, dev, what):
    t = torch.as_tensor(v).reshape(-1).to(torch.int64)
    if t.numel() != B:
        raise ValueError(f"ctc_loss: {what} must have one entry per utterance ({B}), got {t.numel()}")
    return t.cpu(), t.to(dev)


class _CTC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, targets, input_lengths, target_lengths, blank, reduction, zero_infinity, logits):
        L, st = _lib.lib(), _lib.stream_ptr()
        T, B, Cn = x.shape
        dev = x.device
        if x.dtype != torch.float32:
            raise TypeError(f"ctc_loss (HIP): float32 input expected, got {x.dtype}")
        if x.stride(2) != 1:
            x = x.contiguous()
        il_h, il = _lengths(input_lengths, B, dev, "input_lengths")
        tl_h, tl = _lengths(target_lengths, B, dev, "target_lengths")
        if (il_h < 0).any() or (il_h > T).any():
            raise ValueError(f"ctc_loss: input_lengths must lie in [0, {T}]")
        if (tl_h < 0).any():
            raise ValueError("ctc_loss: negative target length")
        max_l = int(tl_h.max()) if B else 0
        if max_l > _MAX_TARGET:
            raise ValueError(f"ctc_loss (HIP): target length {max_l} exceeds the supported {_MAX_TARGET}")
        targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
        if targets.dim() == 2:
            if targets.shape[0] != B or targets.shape[1] < max_l:
                raise ValueError("ctc_loss: padded targets must be (B, S) with S >= max(target_lengths)")
            targets = targets.contiguous()
            tstride = targets.shape[1]
        elif targets.dim() == 1:
            if targets.numel() < int(tl_h.sum()):
                raise ValueError("ctc_loss: 1-D targets shorter than sum(target_lengths)")
            targets = targets.contiguous()
            tstride = 0
        else:
            raise ValueError("ctc_loss: targets must be 1-D (concatenated) or 2-D (padded)")
        if not 0 <= blank < Cn:
            raise ValueError(f"ctc_loss: blank {blank} outside [0, {Cn})")
        need_grad = ctx.needs_input_grad[0]
        wsn = int(L.as_ctc_workspace_floats(T, B, max_l))
        ws = torch.empty(wsn, device=dev, dtype=torch.float32)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        tptr = _lib.ptr(targets) if targets.numel() else C.c_void_p(0)
        args = (_lib.ptr(x), x.stride(0), x.stride(1), T, B, Cn, int(logits), tptr, tstride, _lib.ptr(il), _lib.ptr(tl), max_l, blank)
        _lib.check(L.as_ctc_loss(*args, int(need_grad), _lib.ptr(ws), wsn, _lib.ptr(nll), st), "as_ctc_loss")
        per = nll
        if zero_infinity:
            per = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if reduction == "none":
            out = per
        elif reduction == "sum":
            out = per.sum()
        else:
            out = (per / tl.clamp(min=1).to(per.dtype)).mean()
        if need_grad:
            ctx.save_for_backward(x, targets, il, tl, ws, nll)
            ctx.meta = (args, tstride, max_l, blank, reduction, zero_infinity, wsn, B)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, targets, il, tl, ws, nll = ctx.saved_tensors
        args, tstride, max_l, blank, reduction, zero_infinity, wsn, B = ctx.meta
        gout = gout.float()
        if reduction == "none":
            scale = gout.reshape(B)
        elif reduction == "sum":
            scale = gout.reshape(1).expand(B)
        else:
            scale = gout.reshape(1) / (tl.clamp(min=1).to(torch.float32) * B)
        scale = scale.contiguous()
        grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().as_ctc_grad(*args, _lib.ptr(ws), wsn, _lib.ptr(nll), _lib.ptr(scale), int(zero_infinity), _lib.ptr(grad),
                                          grad.stride(0), grad.stride(1), _lib.stream_ptr()), "as_ctc_grad")
        return grad, None, None, None, None, None, None, None


def ctc_loss(x, targets, input_lengths, target_lengths, blank=0, reduction="mean", zero_infinity=False, logits=False):
    """``torch.nn.functional.ctc_loss`` on the HIP library; ``logits=True`` fuses the log-softmax (see the module docstring)."""
    _lib.require_gpu(x, "x")
    if x.dim() != 3:
        raise ValueError("ctc_loss: x must be (T, B, C)")
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"ctc_loss: unknown reduction {reduction!r}")
    return _CTC.apply(x, targets, input_lengths, target_lengths, int(blank), reduction, bool(zero_infinity), bool(logits))


class CTCLoss(torch.nn.Module):
    """``nn.CTCLoss(blank, reduction, zero_infinity)`` on the kernel (log-probability input, as the reference feeds it)."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ctc_loss(log_probs, targets, input_lengths, target_lengths, self.blank, self.reduction, self.zero_infinity)
