"""Vocal-tract acoustics on the device (csrc/vt_acoustics.hip, as_vt_acoustics): what the tube that the area function describes
sounds like -- its volume-velocity transfer function and its formants, for every frame of a batch in one launch.  The reference
has no acoustic stage (its ``area_function.py`` is imported by nothing): the definition is this project's own, an ASSUMPTION whose
parity with any other synthesiser is unpinned; the header (include/artspeech_hip.h) states it in full.  In short, with lossless
walls and float64 throughout:

- a frame is K tube sections ordered glottis -> lips, area A_i in cm^2 and length l_i in cm; with ``counts`` frame n uses its
  first ``counts[n]`` sections;
- the chain matrix [[A, B], [C, D]] is the product of the sections' matrices at k = 2 pi f / c, z_i = rho c / A_i;
- the radiation load Z is 0 (``radiation="open"``) or Flanagan's piston in a baffle on the last section (``"piston"``);
- den = C Z + D, and the transfer function U_lips / U_glottis is 1 / den;
- the formants are the first ``n_formants`` coarse minima of |den|^2 on the grid f0 + j df, each refined by ``rounds`` rounds of
  64 probes to a bracket 2 df (2 / 65)^rounds wide; the level is -10 log10 |den|^2 at the bracket's midpoint.

Status bits per frame: ``STATUS_CLOSED`` (an area below ``min_area``, a closure as in a stop consonant: computed as ``min_area``,
not an error) and ``STATUS_NON_FINITE`` (a non-finite area or length, a length <= 0 or a count below 1: the frame's outputs are
NaN).  Left out: wall, viscous and heat losses, formant bandwidths, a nasal branch, a time-domain waveform."""
from collections import namedtuple

import torch

from . import _lib

STATUS_CLOSED, STATUS_NON_FINITE = 1, 2
SOUND_SPEED = 35000.0    # cm / s
AIR_DENSITY = 1.14e-3    # g / cm^3
MIN_AREA = 1e-4          # cm^2
RADIATION = {"open": 0, "piston": 1}

Formants = namedtuple("Formants", ["frequencies", "levels", "found", "status"])


def tube_sections(dists, fx, to_cm):
    """The area function's output (..., Nw) -- ``dists`` along the mid line and the areas ``fx`` at its Nw points, in the units of
    the contours -- as Nw - 1 tube sections on the device: areas ``(fx_i + fx_{i+1}) / 2 * to_cm^2`` and lengths
    ``(d_{i+1} - d_i) * to_cm``, float64.  ``to_cm`` is the length of one contour unit in centimetres."""
    _lib.require_gpu(dists, "dists")
    _lib.require_gpu(fx, "fx")
    dists, fx = dists.to(torch.float64), fx.to(torch.float64)
    if dists.shape != fx.shape or dists.shape[-1] < 2:
        raise ValueError(f"tube_sections needs dists and fx of one shape (..., Nw >= 2), got {tuple(dists.shape)} and {tuple(fx.shape)}")
    to_cm = float(to_cm)
    areas = (fx[..., :-1] + fx[..., 1:]) / 2 * (to_cm * to_cm)
    lengths = (dists[..., 1:] - dists[..., :-1]) * to_cm
    return areas, lengths


def _rows(t, name):
    """(tensor, frame stride, section stride) for the kernel: the tensor goes in as it lies when one stride walks its leading
    dimensions (a contiguous tensor, a slice of its last dimension, one row of lengths expanded over the frames); otherwise it is
    made contiguous once."""
    _lib.require_gpu(t, name)
    t = t.detach()
    if t.dtype != torch.float64:
        t = t.to(torch.float64)
    if t.dim() == 1:
        t = t[None]
    try:
        flat = t.view(-1, t.shape[-1])
    except RuntimeError:
        flat = t.contiguous().view(-1, t.shape[-1])
    return flat, flat.stride(0) if flat.shape[0] > 1 else 0, flat.stride(1)


def _launch(areas, lengths, counts, f0, df, n_freq, radiation, c, rho, min_area, n_formants, rounds, want):
    """One as_vt_acoustics launch; ``want`` names the outputs to allocate.  Returns {name: tensor}, the leading dimensions restored."""
    if radiation not in RADIATION and radiation not in (0, 1):
        raise ValueError(f"radiation is one of {sorted(RADIATION)}, got {radiation!r}")
    lead = tuple(areas.shape[:-1])
    if tuple(lengths.shape[-1:]) != tuple(areas.shape[-1:]) or (lengths.dim() > 1 and tuple(lengths.shape) != tuple(areas.shape)):
        raise ValueError(f"areas {tuple(areas.shape)} and lengths {tuple(lengths.shape)} do not describe the same sections")
    if lengths.dim() == 1 and areas.dim() > 1:
        lengths = lengths.expand(areas.shape)
    a, a_frame, a_sec = _rows(areas, "areas")
    l, l_frame, l_sec = _rows(lengths, "lengths")
    n, K = a.shape
    dev = a.device
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if counts.numel() != n:
            raise ValueError(f"counts {tuple(counts.shape)} for {n} frames")
    F, nf = int(n_freq), int(n_formants)
    shapes = {"den": ((n, F), torch.complex128), "transfer": ((n, F), torch.complex128), "freq": ((n, nf), torch.float64),
              "level": ((n, nf), torch.float64), "found": ((n,), torch.int32), "status": ((n,), torch.int32)}
    out = {name: torch.empty(shape, dtype=dtype, device=dev) if name in want else None for name, (shape, dtype) in shapes.items()}
    if n > 0:   # an empty batch launches nothing (and an empty tensor has no address to hand over)
        with torch.cuda.device(dev):
            _lib.call("as_vt_acoustics", a, a_frame, a_sec, l, l_frame, l_sec, counts, n, K, float(f0), float(df), F,
                      RADIATION.get(radiation, radiation), float(c), float(rho), float(min_area), nf, int(rounds), out["den"],
                      out["transfer"], out["freq"], out["level"], out["found"], out["status"])
    return {name: t.reshape(lead + t.shape[1:]) for name, t in out.items() if t is not None}


def transfer_function(areas, lengths, counts=None, f0=10., df=10., n_freq=500, radiation="piston", c=SOUND_SPEED, rho=AIR_DENSITY,
                      min_area=MIN_AREA, return_denominator=False):
    """areas, lengths (..., K) float64 on the GPU (``lengths`` may be one row (K,) for all frames), ``counts`` (...) sections used
    per frame -> the transfer function U_lips / U_glottis, complex128 (..., n_freq), on the grid f0 + j df, and the int32 status
    (...).  ``return_denominator`` adds den = C Z + D = 1 / H behind them."""
    want = ("transfer", "status", "den") if return_denominator else ("transfer", "status")
    out = _launch(areas, lengths, counts, f0, df, n_freq, radiation, c, rho, min_area, 0, 0, want)
    return tuple(out[name] for name in want)


def formants(areas, lengths, counts=None, f0=10., df=10., n_freq=500, radiation="piston", c=SOUND_SPEED, rho=AIR_DENSITY,
             min_area=MIN_AREA, n_formants=5, rounds=3):
    """The formants of every frame: ``Formants(frequencies (..., n_formants) in Hz, levels (..., n_formants) in dB, found (...),
    status (...))``; a slot that was not found holds NaN.  Arguments as for ``transfer_function``."""
    out = _launch(areas, lengths, counts, f0, df, n_freq, radiation, c, rho, min_area, n_formants, rounds,
                  ("freq", "level", "found", "status"))
    return Formants(out["freq"], out["level"], out["found"], out["status"])
