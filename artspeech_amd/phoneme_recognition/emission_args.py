"""The arguments that the recogniser's entry points share, each convention stated once: an emissions tensor, per-utterance
lengths, CTC targets.  Every function validates first, on whatever device its arguments live (shapes, dtypes and host values
only, so a caller may validate before it asks for the GPU), and copies to ``device`` last, when asked."""
import torch

MAX_TARGET = 2047  # target entries of one utterance: S = 2L + 1 <= 4095 states of the CTC recursions (CTC_MAX_L, RE_MAX_L)


def emissions_shape(x, who, time_major, name="emissions"):
    """(T, B, C) of a 3-D emissions tensor laid out (T, B, C) (``time_major``) or (B, T, C)."""
    if x.dim() != 3:
        raise ValueError(f"{who}: {name} must be {'(T, B, C)' if time_major else '(B, T, C)'}")
    t = 0 if time_major else 1
    return x.shape[t], x.shape[1 - t], x.shape[2]


def emissions(x, who, time_major, detach=False, name="emissions"):
    """-> (x, T, B, C, time stride, batch stride), as the library takes emissions: float32, 3-D, in any time and batch strides
    with class stride 1 -- the permuted view of the other layout costs no copy, anything else takes ``.contiguous()``.
    ``detach``: where no gradient is wanted."""
    T, B, C = emissions_shape(x, who, time_major, name)
    if x.dtype != torch.float32:
        raise TypeError(f"{who} (HIP): float32 {name} expected, got {x.dtype}")
    if detach:
        x = x.detach()
    if x.stride(2) != 1:
        x = x.contiguous()
    t = 0 if time_major else 1
    return x, T, B, C, x.stride(t), x.stride(1 - t)


def lengths(v, B, who, what="lengths", T=None, host=False, device=None):
    """One int64 entry per utterance -> (the lengths, their copy on ``device`` or None).  The first stays where ``v`` is unless
    ``host`` or a range check asks for the host copy; ``T``: every length must lie in [0, T]."""
    t = torch.as_tensor(v).reshape(-1).to(torch.int64)
    if t.numel() != B:
        raise ValueError(f"{who}: {what} must have one entry per utterance ({B}), got {t.numel()}")
    first = t.cpu() if host or T is not None else t
    if T is not None and ((first < 0).any() or (first > T).any()):
        raise ValueError(f"{who}: {what} must lie in [0, {T}]")
    return first, None if device is None else t.to(device)


def ctc_targets(targets, target_lengths, B, who, blank, n_classes, device=None):
    """CTC targets, padded (B, S) or torch's 1-D concatenated form, with their host lengths -> (the int64 targets on ``device``,
    None when empty; tstride: the row pitch, 0 = concatenated; max_l).  At most MAX_TARGET entries per utterance; the blank
    lies inside the classes."""
    if (target_lengths < 0).any():
        raise ValueError(f"{who}: negative target length")
    max_l = int(target_lengths.max()) if B else 0
    if max_l > MAX_TARGET:
        raise ValueError(f"{who} (HIP): target length {max_l} exceeds the supported {MAX_TARGET}")
    targets = torch.as_tensor(targets)
    if targets.dim() == 2:
        if targets.shape[0] != B or targets.shape[1] < max_l:
            raise ValueError(f"{who}: padded targets must be (B, S) with S >= max(target_lengths)")
        tstride = targets.shape[1]
    elif targets.dim() == 1:
        if targets.numel() < int(target_lengths.sum()):
            raise ValueError(f"{who}: 1-D targets shorter than sum(target_lengths)")
        tstride = 0
    else:
        raise ValueError(f"{who}: targets must be 1-D (concatenated) or 2-D (padded)")
    if not 0 <= blank < n_classes:
        raise ValueError(f"{who}: blank {blank} outside [0, {n_classes})")
    targets = targets.to(device=device, dtype=torch.int64).contiguous()
    return (targets if targets.numel() else None), tstride, max_l
