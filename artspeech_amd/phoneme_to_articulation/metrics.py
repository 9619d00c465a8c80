"""Losses of the path on MI355X (reference: phoneme_to_articulation/metrics.py).

``EuclideanDistance`` (:5-24) and ``MeanP2CPDistance`` (:27-46) keep the reference's constructor and
call signatures, including the ``reduction = getattr(torch, name, identity)`` convention ("none" ->
identity, "mean" -> torch.mean, ...).  ``masked_euclidean_loss`` is the fused form of the training
loop's criterion + padding mask + mean (train_phoneme_to_articulation.py:86-90); ``masked_p2cp_loss`` is the same with
``MeanP2CPDistance`` as the criterion.  Both criteria are differentiable, as in the reference.
"""
import torch
import torch.nn as nn

from .. import _lib


class _EuclidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, targets):
        A, two, N = outputs.shape[-3:]
        frames = outputs.numel() // (A * 2 * N)
        o, t = outputs.contiguous(), targets.contiguous()
        dist = torch.empty((*outputs.shape[:-2], N), dtype=torch.float32, device=outputs.device)
        _lib.call("as_euclid_fwd", o, t, frames, A, N, dist)
        ctx.save_for_backward(o, t)
        ctx.dims = (frames, A, N)
        return dist

    @staticmethod
    def backward(ctx, ddist):
        o, t = ctx.saved_tensors
        frames, A, N = ctx.dims
        dout = torch.empty_like(o)
        ddist = ddist.contiguous()  # named: must stay alive until the launch is enqueued
        _lib.call("as_euclid_bwd", o, t, ddist, frames, A, N, dout)
        return dout, (-dout if ctx.needs_input_grad[1] else None)


def _check_pair(outputs, targets):
    _lib.require_gpu(outputs, "outputs")
    _lib.require_gpu(targets, "targets")
    if outputs.shape != targets.shape or outputs.dim() < 3 or outputs.shape[-2] != 2:
        raise RuntimeError(f"expected two tensors of shape (..., N_art, 2, N_samples), got {tuple(outputs.shape)} "
                           f"and {tuple(targets.shape)}")
    if outputs.dtype != torch.float32 or targets.dtype != torch.float32:
        raise RuntimeError("artspeech_amd metrics compute in float32")


class EuclideanDistance(nn.Module):
    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction_name = reduction
        self.reduction = getattr(torch, reduction, lambda x: x)

    def forward(self, outputs, targets):
        """
        Args:
        outputs (torch.tensor): Torch tensor with shape (bs, seq_len, N_art, 2, N_samples).
        targets (torch.tensor): Torch tensor with shape (bs, seq_len, N_art, 2, N_samples).
        """
        _check_pair(outputs, targets)
        return self.reduction(_EuclidFn.apply(outputs, targets))


class _MaskedLossFn(torch.autograd.Function):
    """as_<kind>_masked_fwd_bwd, kind "euclid" or "p2cp": the two fused criteria share their signature."""

    @staticmethod
    def forward(ctx, outputs, targets, lengths_dev, scale, kind):
        B, T, A, _, N = outputs.shape
        o, t = outputs.contiguous(), targets.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=o.device)
        need_grad = bool(ctx.needs_input_grad[0])
        dout = torch.empty_like(o) if need_grad else None
        p2cp = kind == "p2cp"
        n_partial = _lib.call("as_p2cp_masked_partials" if p2cp else "as_euclid_masked_partials")
        partial = torch.empty(n_partial, dtype=torch.float32, device=o.device)
        _lib.call("as_p2cp_masked_fwd_bwd" if p2cp else "as_euclid_masked_fwd_bwd", o, t, t.shape[1], lengths_dev, B, T, A, N, float(scale),
                  loss, dout, partial)
        if need_grad:
            ctx.save_for_backward(dout)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dout,) = ctx.saved_tensors
        return dout * dloss, None, None, None, None


def _masked_loss(kind, outputs, targets, lengths, n_valid_global, terms_per_frame):
    _check_pair(outputs[:, :1], targets[:, :1])
    lengths_cpu = torch.as_tensor(lengths, dtype=torch.int32, device="cpu")
    n_valid = int(lengths_cpu.sum()) if n_valid_global is None else int(n_valid_global)
    scale = 1.0 / (n_valid * terms_per_frame)
    return _MaskedLossFn.apply(outputs, targets, lengths_cpu.to(outputs.device, non_blocking=True), scale, kind)


def masked_euclidean_loss(outputs, targets, lengths, n_valid_global=None):
    """mean over {valid frames} x articulators x points of the Euclidean distance -- the criterion,
    padding mask and mean of train_phoneme_to_articulation.py:86-90 in one kernel (its gradient comes
    out of the same pass).  targets may be padded longer than outputs (T_out = max(lengths)).
    n_valid_global: total number of valid frames of the GLOBAL batch when this rank holds a shard
    (data parallel): shard losses then SUM to the reference's global mean."""
    A, N = outputs.shape[2], outputs.shape[4]
    return _masked_loss("euclid", outputs, targets, lengths, n_valid_global, A * N)


def masked_p2cp_loss(outputs, targets, lengths, n_valid_global=None):
    """mean over {valid frames} x articulators of the point-to-closest-point distance between the predicted and the target
    contour -- MeanP2CPDistance("none") on the (.., 2, N) storage, the padding mask and the mean of
    train_phoneme_to_articulation.py:86-90 in one kernel, its gradient out of the same pass (targets are constants; up to
    256 points per contour).  Padded frames are never read.  lengths / n_valid_global: as masked_euclidean_loss."""
    return _masked_loss("p2cp", outputs, targets, lengths, n_valid_global, outputs.shape[2])


def _planar_strides(t):
    """(tile, point, xy) element strides of a (*, n, 2) tensor if its batch dims collapse to one
    uniform tile stride, else None."""
    n = t.shape[-2]
    if t.dim() == 2:
        return 0, t.stride(0), t.stride(1)
    lead_shape, lead_strides = t.shape[:-2], t.stride()[:-2]
    tile = lead_strides[-1]
    expect = tile
    for size, stride in zip(reversed(lead_shape), reversed(lead_strides)):
        if size != 1 and stride != expect:
            return None
        expect = stride * size if size != 1 else expect
    return tile, t.stride(-2), t.stride(-1)


def _p2cp_operands(u_, v_):
    """The pair as as_p2cp_fwd / as_p2cp_bwd address it: (u_, strides, v_, strides), a copy only where the batch dims of a
    tensor do not collapse to one tile stride."""
    su, sv = _planar_strides(u_), _planar_strides(v_)
    if su is None:
        u_ = u_.contiguous()
        su = _planar_strides(u_)
    if sv is None:
        v_ = v_.contiguous()
        sv = _planar_strides(v_)
    return u_, su, v_, sv


def _p2cp_fwd(u_, su, v_, sv):
    lead = u_.shape[:-2]
    tiles = 1
    for s in lead:
        tiles *= s
    out = torch.empty(lead, dtype=torch.float32, device=u_.device)
    with torch.no_grad():
        _lib.call("as_p2cp_fwd", u_, su[0], su[1], su[2], u_.shape[-2], v_, sv[0], sv[1], sv[2], v_.shape[-2], tiles, out)
    return out


def _grad_like(t, strides):
    """An uninitialised gradient of t's shape (*, n, 2): on (*, 2, n) storage, handed out as its transposed view, when t is
    such a view itself (the kernel's lanes then write consecutive floats), contiguous otherwise."""
    if strides[1] == 1 and strides[2] != 1:
        return torch.empty((*t.shape[:-2], 2, t.shape[-2]), dtype=torch.float32, device=t.device).transpose(-1, -2)
    return torch.empty(t.shape, dtype=torch.float32, device=t.device)


class _P2CPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u_, v_):
        u_, su, v_, sv = _p2cp_operands(u_, v_)
        ctx.save_for_backward(u_, v_)
        ctx.strides = (su, sv)
        return _p2cp_fwd(u_, su, v_, sv)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        u_, v_ = ctx.saved_tensors
        su, sv = ctx.strides
        dout = dout.contiguous().float()  # named: must stay alive until the launch is enqueued
        du = _grad_like(u_, su) if ctx.needs_input_grad[0] else None   # only the sides that need a gradient
        dv = _grad_like(v_, sv) if ctx.needs_input_grad[1] else None
        sdu = _planar_strides(du) if du is not None else (0, 0, 0)
        sdv = _planar_strides(dv) if dv is not None else (0, 0, 0)
        _lib.call("as_p2cp_bwd", u_, su[0], su[1], su[2], u_.shape[-2], v_, sv[0], sv[1], sv[2], v_.shape[-2], dout.numel(), dout, du,
                  sdu[0], sdu[1], sdu[2], dv, sdv[0], sdv[1], sdv[2])
        return du, dv


def mean_p2cp(u_, v_):
    """MeanP2CPDistance, reduction "none": u_ (*, N, 2), v_ (*, M, 2) -> (*).  Transposed views of
    (*, 2, N) storage (how the reference calls it: metrics.py:47-50, encoder_decoder/metrics.py:19-22)
    are consumed in place through strides, no copy.  Differentiable like the reference's (cdist -> min): with grad mode on
    and an input that requires grad the gradient is as_p2cp_bwd's -- the closest points of the forward's own arithmetic,
    the lowest index among equally close ones (torch.min), nothing from a coincident pair (cdist's backward, no NaN)."""
    _lib.require_gpu(u_, "u_")
    _lib.require_gpu(v_, "v_")
    if u_.shape[-1] != 2 or v_.shape[-1] != 2 or u_.shape[:-2] != v_.shape[:-2]:
        raise RuntimeError(f"expected (*, N, 2) and (*, M, 2), got {tuple(u_.shape)} and {tuple(v_.shape)}")
    if torch.is_grad_enabled() and (u_.requires_grad or v_.requires_grad):
        return _P2CPFn.apply(u_, v_)
    return _p2cp_fwd(*_p2cp_operands(u_, v_))


class MeanP2CPDistance(nn.Module):
    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction_name = reduction
        self.reduction = getattr(torch, reduction, lambda x: x)

    def forward(self, u_, v_):
        """
        Args:
        u_ (torch.tensor): Tensor of shape (*, N, 2)
        v_ (torch.tensor): Tensor of shape (*, M, 2)
        """
        return self.reduction(mean_p2cp(u_, v_))
