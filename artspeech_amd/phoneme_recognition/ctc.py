"""CTC loss on the HIP library (as_ctc_loss / as_ctc_grad): a drop-in for ``torch.nn.CTCLoss`` as the reference calls it,
``criterion(log_softmax(outputs).permute(1, 0, 2), targets, input_lengths, target_lengths)`` (phoneme_recognition/__init__.py:
112-120).

``ctc_loss(x, ...)`` takes the (T, B, C) rows in any strides whose class stride is 1 -- the permuted view of a (B, T, C) tensor
costs no copy -- and targets either padded (B, S) (the reference's collate pads them with -1) or torch's concatenated 1-D form.
``logits=False``: x holds log-probabilities (torch semantics); ``logits=True``: x holds raw scores and the kernel normalises them
itself, so a trainer can skip the log-softmax pass: the gradient is then taken with respect to the scores.  Reductions and
``zero_infinity`` follow torch: ``mean`` divides each utterance's loss by max(target_length, 1), then averages over the batch.
"""
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
        wsn = int(_lib.call("as_ctc_workspace_floats", T, B, max_l))
        ws = torch.empty(wsn, device=dev, dtype=torch.float32)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        tgt = targets if targets.numel() else None
        _lib.call("as_ctc_loss", x, x.stride(0), x.stride(1), T, B, Cn, int(logits), tgt, tstride, il, tl, max_l, blank, int(need_grad),
                  ws, wsn, nll)
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
            ctx.meta = (int(logits), tstride, max_l, blank, reduction, zero_infinity, wsn)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, targets, il, tl, ws, nll = ctx.saved_tensors
        logits, tstride, max_l, blank, reduction, zero_infinity, wsn = ctx.meta
        T, B, Cn = x.shape
        gout = gout.float()
        if reduction == "none":
            scale = gout.reshape(B)
        elif reduction == "sum":
            scale = gout.reshape(1).expand(B)
        else:
            scale = gout.reshape(1) / (tl.clamp(min=1).to(torch.float32) * B)
        scale = scale.contiguous()
        grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        tgt = targets if targets.numel() else None
        _lib.call("as_ctc_grad", x, x.stride(0), x.stride(1), T, B, Cn, logits, tgt, tstride, il, tl, max_l, blank, ws, wsn, nll, scale,
                  int(zero_infinity), grad, grad.stride(0), grad.stride(1))
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
