"""B-spline smoothing of contours on the device (csrc/contour_spline.hip, as_contour_spline): every contour of a batch in one
launch.  The reference smooths each predicted contour with ``vt_tools.bs_regularization.regularize_Bsplines(contour, 3)`` before
it saves it (generate_vocal_tract_shape_v2.py:173,252, generate_vocal_tract_shape.py:155, phoneme_to_articulation/__init__.py:
178-180).  ``vt_tools`` is neither vendored nor pinned: the definition here -- a chord-length parameter, a clamped
uniform knot vector, a least-squares fit with a second-difference penalty on the control points, solved in float64 -- is this
project's own, an ASSUMPTION whose parity with ``vt_tools`` is unpinned, as ``load_articulator_array`` says of its package."""
import numpy as np
import torch

from .. import _lib

STATUS_ZERO_LENGTH = 1   # bit 0 of a contour's status: all its points coincide, every output is the first point
STATUS_NON_FINITE = 2    # bit 1: a NaN or infinite coordinate, the contour's outputs are NaN


def _contour_stride(x):
    """The one element stride that walks the leading dimensions of x (..., 2, N) as a flat contour index, or None."""
    dims = [(n, s) for n, s in zip(x.shape[:-2], x.stride()[:-2]) if n != 1]
    for (_, s0), (n1, s1) in zip(dims, dims[1:]):
        if s0 != s1 * n1:
            return None
    return dims[-1][1] if dims else 0


def regularize_contours(contours, degree=3, n_ctrl=12, smoothing=1e-3, n_out=None, lengths=None, return_status=False):
    """contours (..., 2, N) float32 on the GPU -> (..., 2, n_out or N) float32: each contour replaced by ``n_out`` points of its
    smoothing spline of ``degree`` with ``n_ctrl`` control points and penalty weight ``smoothing`` (> 0).  The tensor goes in as
    it lies when one stride walks its leading dimensions ((B, T, A, 2, N) model outputs, a permuted view of (F, A, N, 2) raw
    contours); otherwise it is made contiguous once.  With ``lengths`` (B,) the leading dimensions are (B, T, A) and the contours
    of frames t >= lengths[b] come back as zeros.  ``return_status`` adds the int32 flags (...,) (STATUS_* bits).  Limits
    (2 <= N <= 256, degree + 1 <= n_ctrl <= 32, 2 <= n_out <= 1024, degree 1 .. 3) are refused by the library, not truncated."""
    _lib.require_gpu(contours, "contours")
    if contours.dim() < 2 or contours.shape[-2] != 2:
        raise ValueError(f"regularize_contours needs (..., 2, N) contours, got {tuple(contours.shape)}")
    x = contours.detach()
    if x.dtype != torch.float32:
        x = x.float()
    s_contour = _contour_stride(x)
    if s_contour is None:
        x = x.contiguous()
        s_contour = _contour_stride(x)
    lead, N = tuple(x.shape[:-2]), x.shape[-1]
    M = N if n_out is None else int(n_out)
    n = int(np.prod(lead, dtype=np.int64))
    T = A = 0
    if lengths is not None:
        if len(lead) != 3:
            raise ValueError(f"with lengths the contours are (B, T, A, 2, N), got {tuple(contours.shape)}")
        lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int64).contiguous()
        if lengths.shape != (lead[0],):
            raise ValueError(f"lengths {tuple(lengths.shape)} for a batch of {lead[0]}")
        T, A = lead[1], lead[2]
    out = torch.empty(lead + (2, M), dtype=torch.float32, device=x.device)
    status = torch.empty(lead, dtype=torch.int32, device=x.device) if return_status else None
    if n == 0:
        return (out, status) if return_status else out
    with torch.cuda.device(x.device):
        _lib.call("as_contour_spline", x, s_contour, x.stride(-2), x.stride(-1), n, N, int(n_ctrl), int(degree), float(smoothing), M,
                  lengths, T, A, out, M, status)
    return (out, status) if return_status else out


def regularize_Bsplines(contour, degree, n_ctrl=12, smoothing=1e-3, n_out=None):
    """The reference's call form, for callers that port a line at a time: an (N, 2) array -> (reg_X, reg_Y) numpy arrays.  One
    launch and two copies per contour: a batch belongs to ``regularize_contours``."""
    if not torch.cuda.is_available():
        raise RuntimeError("artspeech_amd smooths contours on an MI355X device; there is no CPU path")
    points = torch.as_tensor(np.asarray(contour, dtype=np.float32))
    if points.dim() != 2 or points.shape[1] != 2:
        raise ValueError(f"regularize_Bsplines needs an (N, 2) contour, got {tuple(points.shape)}")
    dev = torch.device("cuda", torch.cuda.current_device())
    reg = regularize_contours(points.to(dev).T, degree, n_ctrl, smoothing, n_out).cpu().numpy()
    return reg[0], reg[1]
