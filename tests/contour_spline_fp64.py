"""Test infrastructure only: the restatement of the contour smoothing in plain numpy float64, the contract of
artspeech_amd/csrc/contour_spline.hip (include/artspeech_hip.h, as_contour_spline).  A hand-written Cox-de Boor recursion, the dense
normal equations and ``numpy.linalg.solve``; nothing here is shared with the package.

One contour of N points p_i, degree d, K control points, M outputs:
  s_0 = 0, s_i = s_{i-1} + |p_i - p_{i-1}|, u_i = s_i / s_{N-1}, u_{N-1} = 1; s_{N-1} == 0 -> every output is p_0
  knots [0]*d + linspace(0, 1, K-d+1) + [1]*d, span(u) = min(floor(u (K-d)), K-d-1)
  (B'B + lambda D'D) c = B'p, D the (K-2, K) second difference; S(m / (M-1)) for m = 0 .. M-1."""
import numpy as np


def knot_vector(K, d):
    return np.concatenate([np.zeros(d), np.linspace(0.0, 1.0, K - d + 1), np.ones(d)])


def span_of(u, K, d):
    return min(int(np.floor(u * (K - d))), K - d - 1)


def basis_row(u, K, d, knots=None):
    """(span, the d + 1 values of the basis functions span .. span + d at u): the triangular Cox-de Boor scheme."""
    kt = knot_vector(K, d) if knots is None else knots
    span = span_of(u, K, d)
    k = span + d
    nb = np.zeros(d + 1)
    left, right = np.zeros(d + 1), np.zeros(d + 1)
    nb[0] = 1.0
    for j in range(1, d + 1):
        left[j] = u - kt[k + 1 - j]
        right[j] = kt[k + j] - u
        saved = 0.0
        for r in range(j):
            temp = nb[r] / (right[r + 1] + left[j - r])
            nb[r] = saved + right[r + 1] * temp
            saved = left[j - r] * temp
        nb[j] = saved
    return span, nb


def design_matrix(u, K, d):
    """Dense (len(u), K) collocation matrix."""
    kt = knot_vector(K, d)
    B = np.zeros((len(u), K))
    for i, ui in enumerate(u):
        span, nb = basis_row(float(ui), K, d, kt)
        B[i, span:span + d + 1] = nb
    return B


def parameter(points):
    """u (N,) of points (N, 2) float64, or None for a contour of zero length."""
    seg = np.sqrt((np.diff(points, axis=0) ** 2).sum(axis=1))
    s = np.concatenate([[0.0], np.cumsum(seg)])
    if s[-1] == 0.0:
        return None
    u = s / s[-1]
    u[-1] = 1.0
    return u


def second_difference(K):
    D = np.zeros((max(K - 2, 0), K))
    for m in range(K - 2):
        D[m, m:m + 3] = (1.0, -2.0, 1.0)
    return D


def normal_matrix(points, K, d, lam):
    """The matrix of the fit of one contour (for the conditioning assertion); None for zero length."""
    u = parameter(np.asarray(points, dtype=np.float64))
    if u is None:
        return None
    B, D = design_matrix(u, K, d), second_difference(K)
    return B.T @ B + lam * (D.T @ D)


def smooth(points, degree=3, n_ctrl=12, lam=1e-3, n_out=None):
    """points (N, 2) array-like -> (2, M) float64 (x row, y row); float32 inputs are widened first, nothing is rounded."""
    p = np.asarray(points, dtype=np.float64)
    N = p.shape[0]
    M = N if n_out is None else n_out
    if not np.isfinite(p).all():
        return np.full((2, M), np.nan)
    u = parameter(p)
    if u is None:
        return np.repeat(p[0][:, None], M, axis=1)
    B, D = design_matrix(u, n_ctrl, degree), second_difference(n_ctrl)
    c = np.linalg.solve(B.T @ B + lam * (D.T @ D), B.T @ p)
    v = np.arange(M) / (M - 1)
    v[-1] = 1.0
    return (design_matrix(v, n_ctrl, degree) @ c).T


def smooth_batch(contours, degree=3, n_ctrl=12, lam=1e-3, n_out=None):
    """contours (..., 2, N) -> (..., 2, M) float64."""
    x = np.asarray(contours)
    lead = x.shape[:-2]
    flat = x.reshape((-1,) + x.shape[-2:])
    out = np.stack([smooth(c.T, degree, n_ctrl, lam, n_out) for c in flat])
    return out.reshape(lead + out.shape[-2:])


# The shapes of the device parity test, the smallest that can go wrong: (contours, N, K or None for degree + 1, degree, M, lambda).
# N: one point per lane (2, 3, 50, 64), then the second pass (65) and the limit (256); contours: inside one workgroup's four waves
# (1, 4), across workgroups (5, 257); M likewise.  The pairs avoid what the definition itself makes ill-conditioned (2 or 3 points
# against 12 or 32 control points at lambda = 1e-6: condition 1e8 .. 1e10): tests/test_contour_spline_host.py asserts <= 1e8 for all.
PARITY_CASES = [
    (1, 2, None, 1, 2, 1.0),
    (4, 2, None, 3, 50, 1e-6),
    (5, 3, None, 2, 64, 1e-3),
    (5, 3, 12, 3, 65, 1.0),
    (257, 50, 12, 3, 50, 1e-3),
    (5, 50, None, 1, 50, 1e-3),
    (4, 50, 32, 2, 1024, 1e-3),
    (5, 64, 12, 1, 65, 1e-6),
    (4, 64, 32, 3, 64, 1e-3),
    (5, 65, 12, 2, 2, 1e-6),
    (4, 65, 32, 1, 50, 1.0),
    (4, 256, 12, 2, 65, 1e-3),
    (5, 256, 32, 3, 1024, 1e-6),
    (1, 256, None, 3, 64, 1.0),
]
DEFAULTS = (3, 12, 1e-3)   # degree, control points, lambda of regularize_contours: what the layout and edge-case tests use


def case_contours(n, N, seed=0):
    """(n, 2, N) float32: smooth, clustered and repeated-point contours in turn, none of zero length."""
    rng = np.random.default_rng(seed + 1000 * N + n)
    makers = (smooth_curve, clustered_contour, repeated_contour)
    out = []
    while len(out) < n:
        pts = makers[len(out) % 3](rng, N)
        if parameter(pts.astype(np.float64)) is not None:
            out.append(pts.T)
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def clustered_contour(rng, N):
    """N points in the unit square, most of them bunched: arc-length parameters that leave some knot spans almost empty."""
    t = np.sort(rng.random(N) ** 3)
    t = np.where(rng.random(N) < 0.5, t, t[rng.integers(0, N, N)])
    t = np.sort(t)
    return np.stack([0.5 + 0.4 * np.cos(3.0 * t), 0.5 + 0.4 * np.sin(2.0 * t) * t], axis=1).astype(np.float32)


def repeated_contour(rng, N):
    """A smooth contour with runs of repeated points (zero-length chords)."""
    base = smooth_curve(rng, max(2, N // 3))
    idx = np.sort(rng.integers(0, base.shape[0], N))
    return base[idx]


def smooth_curve(rng, N):
    """A gently noisy open curve in the unit square, like a model's contour."""
    t = np.linspace(0.0, 1.0, N)
    a, b = rng.uniform(0.5, 2.5, 2)
    x = 0.5 + 0.35 * np.cos(a * np.pi * t) + 0.01 * rng.standard_normal(N)
    y = 0.5 + 0.35 * np.sin(b * np.pi * t) + 0.01 * rng.standard_normal(N)
    return np.stack([x, y], axis=1).astype(np.float32)
