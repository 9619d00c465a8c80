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
from . import emission_args as args


class _CTC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, targets, input_lengths, target_lengths, blank, reduction, zero_infinity, logits):
        x, T, B, Cn, st, sb = args.emissions(x, "ctc_loss", True, name="x")
        dev = x.device
        _, il = args.lengths(input_lengths, B, "ctc_loss", "input_lengths", T=T, device=dev)
        tl_h, tl = args.lengths(target_lengths, B, "ctc_loss", "target_lengths", host=True, device=dev)
        targets, tstride, max_l = args.ctc_targets(targets, tl_h, B, "ctc_loss", blank, Cn, dev)
        need_grad = ctx.needs_input_grad[0]
        wsn = int(_lib.call("as_ctc_workspace_floats", T, B, max_l))
        ws = torch.empty(wsn, device=dev, dtype=torch.float32)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        _lib.call("as_ctc_loss", x, st, sb, T, B, Cn, int(logits), targets, tstride, il, tl, max_l, blank, int(need_grad), ws, wsn, nll)
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
            ctx.meta = (int(logits), tstride, max_l, blank, reduction, zero_infinity, wsn, st, sb)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, targets, il, tl, ws, nll = ctx.saved_tensors
        logits, tstride, max_l, blank, reduction, zero_infinity, wsn, st, sb = ctx.meta
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
        _lib.call("as_ctc_grad", x, st, sb, T, B, Cn, logits, targets, tstride, il, tl, max_l, blank, ws, wsn, nll, scale,
                  int(zero_infinity), grad, grad.stride(0), grad.stride(1))
        return grad, None, None, None, None, None, None, None


def ctc_loss(x, targets, input_lengths, target_lengths, blank=0, reduction="mean", zero_infinity=False, logits=False):
    """``torch.nn.functional.ctc_loss`` on the HIP library; ``logits=True`` fuses the log-softmax (see the module docstring)."""
    _lib.require_gpu(x, "x")
    args.emissions_shape(x, "ctc_loss", True, "x")
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
