"""The vocal-tract tube on the device (csrc/vocal_tract_tube.hip, as_vocal_tract_tube): the internal and the external wall of every
frame of a batch in one launch -- the link between the ``inference_contours/`` that the synthesis writes and the ``air_column/``
that the area function and the recogniser's ``Feature.AIR_COLUMN`` read.  The reference calls
``vt_shape_gen.vocal_tract_tube.generate_vocal_tract_tube`` (generate_vocal_tract_shape_v2.py:426, generate_vocal_tract_shape.py:34,
scripts/shape_to_air_column.py:77).  ``vt_shape_gen`` is neither vendored nor pinned: the definition here is this
project's own, an ASSUMPTION whose parity with ``vt_shape_gen`` is unpinned, as ``regularization.py`` says of its package.

A wall is built from a chain of K <= 8 articulator contours of N points each; nothing depends on the orientation in which a
contour is stored.

- Junctions: for consecutive contours c_k, c_{k+1} the pair (i_k, j_k) that minimises |c_k[i] - c_{k+1}[j]|^2 (float32,
  ``dx*dx + dy*dy`` uncontracted), the first minimum in row-major order.
- Runs: contour k contributes its points from its entry (j_{k-1}) to its exit (i_k), in whichever direction that is.  The first
  contour starts at the end that leaves more points before its exit (a tie: index 0), the last one ends at the end that leaves
  more points behind its entry (a tie: index N-1); a chain of one contour is that contour from 0 to N-1.
- Resampling, in float64: ``n_out`` points at equal steps of arc length along the concatenated runs (the jump between two contours
  is a segment like any other), the first and the last point copied.
- Status, per wall: ``STATUS_ZERO_LENGTH`` (all points coincide: every output is the first point), ``STATUS_NON_FINITE`` (a NaN or
  infinite coordinate in a chain contour: NaN outputs, junctions -1).

The default chains are ASSUMPTIONS too: the articulators that bound the air column from below and from above, from the glottis to
the lips."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .regularization import STATUS_NON_FINITE, STATUS_ZERO_LENGTH, _contour_stride  # noqa: F401  (the bits mean the same here)

INTERNAL_WALL = ("vocal-folds", "thyroid-cartilage", "epiglottis", "tongue", "lower-incisor", "lower-lip")
EXTERNAL_WALL = ("vocal-folds", "arytenoid-cartilage", "pharynx", "soft-palate-midline", "upper-incisor", "upper-lip")
MAX_CHAIN = 8   # VTT_MAX_K of the kernel


def chain_indices(articulators, chain, name="chain"):
    """The channels of ``chain``'s articulators in ``articulators``; one that the data does not have is dropped, and a chain left
    empty (or one longer than the kernel takes) raises ValueError."""
    articulators = list(articulators)
    picked = [articulators.index(a) for a in chain if a in articulators]
    if not picked:
        raise ValueError(f"the {name} wall has none of its articulators ({', '.join(chain)}) among {articulators}")
    if len(picked) > MAX_CHAIN:
        raise ValueError(f"the {name} wall chains {len(picked)} articulators; at most {MAX_CHAIN} are supported")
    return picked


def vocal_tract_tube(contours, articulators, internal=INTERNAL_WALL, external=EXTERNAL_WALL, n_out=100, lengths=None,
                     return_status=False, return_junctions=False, return_length=False):
    """contours (..., A, 2, N) float32 on the GPU, ``articulators`` the name of each of the A channels -> the air columns
    (..., 2, 2, n_out) float64: walls (internal first), coordinates, points -- the air-column file layout, which
    ``area_function_batched`` and ``intersect_semipolar_grid_batched`` take as it comes.  The tensor goes in as it lies when one
    stride walks its leading dimensions ((B, T, A, 2, N) model outputs, a permuted view of (F, A, N, 2) raw contours); otherwise it
    is made contiguous once.  With ``lengths`` (B,) the leading dimensions are (B, T) and the frames t >= lengths[b] come back as
    zeros (status 0, junctions -1, length 0).  ``return_status`` adds int32 (..., 2) STATUS_* bits, ``return_junctions`` int32
    (..., 2, 7, 2) (i_k, j_k) with -1 for the unused ones, ``return_length`` float64 (..., 2) arc lengths, in this order.  Limits
    (2 <= N <= 128, chains of 1 .. 8, 2 <= n_out <= 1024) are refused by the library, not truncated."""
    _lib.require_gpu(contours, "contours")
    if contours.dim() < 3 or contours.shape[-2] != 2 or contours.shape[-3] != len(articulators):
        raise ValueError(f"vocal_tract_tube needs (..., {len(articulators)}, 2, N) contours, got {tuple(contours.shape)}")
    k_int, k_ext = chain_indices(articulators, internal, "internal"), chain_indices(articulators, external, "external")
    x = contours.detach()
    if x.dtype != torch.float32:
        x = x.float()
    frames_view = x.select(-3, 0)   # (..., 2, N): the leading dimensions walk like a contour's
    s_frame = _contour_stride(frames_view)
    if s_frame is None:
        x = x.contiguous()
        s_frame = _contour_stride(x.select(-3, 0))
    lead, A, N = tuple(x.shape[:-3]), x.shape[-3], x.shape[-1]
    M = int(n_out)
    n = int(np.prod(lead, dtype=np.int64))
    T = 0
    if lengths is not None:
        if len(lead) != 2:
            raise ValueError(f"with lengths the contours are (B, T, A, 2, N), got {tuple(contours.shape)}")
        lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int64).contiguous()
        if lengths.shape != (lead[0],):
            raise ValueError(f"lengths {tuple(lengths.shape)} for a batch of {lead[0]}")
        T = lead[1]
    air = torch.empty(lead + (2, 2, M), dtype=torch.float64, device=x.device)
    status = torch.empty(lead + (2,), dtype=torch.int32, device=x.device) if return_status else None
    junctions = torch.empty(lead + (2, MAX_CHAIN - 1, 2), dtype=torch.int32, device=x.device) if return_junctions else None
    length = torch.empty(lead + (2,), dtype=torch.float64, device=x.device) if return_length else None
    if n > 0:
        chains = (ctypes.c_int32 * (2 * MAX_CHAIN))(*([-1] * (2 * MAX_CHAIN)))   # on the host: the library checks and copies it
        chains[:len(k_int)] = k_int
        chains[MAX_CHAIN:MAX_CHAIN + len(k_ext)] = k_ext
        with torch.cuda.device(x.device):
            _lib.call("as_vocal_tract_tube", x, s_frame, x.stride(-3), x.stride(-2), x.stride(-1), n, A, N, chains, len(k_int),
                      len(k_ext), lengths, T, M, air, M, status, junctions, length)
    extras = [t for t, on in ((status, return_status), (junctions, return_junctions), (length, return_length)) if on]
    return (air, *extras) if extras else air


def _as_contour(value):
    """A (2, N) float32 array from a .npy filepath, a (2, N) or an (N, 2) array ((2, 2): taken as (2, N), coordinates first)."""
    array = np.load(value) if isinstance(value, (str, bytes)) or hasattr(value, "__fspath__") else np.asarray(value)
    array = np.asarray(array, dtype=np.float32)
    if array.ndim != 2 or 2 not in array.shape:
        raise ValueError(f"a contour is a (2, N) or (N, 2) array, got {array.shape}")
    return array if array.shape[0] == 2 else array.T


def generate_vocal_tract_tube(articulators_dict, norm_value=None, n_out=100):
    """The reference's call form, for callers that port a line at a time: {articulator: .npy filepath or (2, N) / (N, 2) array} ->
    (internal_wall, external_wall), two (n_out, 2) numpy float64 arrays as ``save_air_column`` and ``area_function`` take them.
    Coordinates are divided by ``norm_value`` when it is given -- an ASSUMPTION: scripts/shape_to_air_column.py:77-80 passes the
    image resolution.  One launch and two copies per frame: a batch belongs to ``vocal_tract_tube``."""
    if not torch.cuda.is_available():
        raise RuntimeError("artspeech_amd builds the vocal-tract tube on an MI355X device; there is no CPU path")
    names = sorted(articulators_dict)
    arrays = [_as_contour(articulators_dict[a]) for a in names]
    if len({a.shape for a in arrays}) != 1:
        raise ValueError(f"the contours of one frame have one point count, got {sorted({a.shape[1] for a in arrays})}")
    frame = np.stack(arrays)
    if norm_value is not None:
        frame = frame / np.float32(norm_value)
    dev = torch.device("cuda", torch.cuda.current_device())
    air = vocal_tract_tube(torch.from_numpy(frame).to(dev), names, n_out=n_out).cpu().numpy()
    return air[0].T.copy(), air[1].T.copy()
