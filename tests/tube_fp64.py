"""The vocal-tract tube restated in numpy (the definition at the top of csrc/vocal_tract_tube.hip): the junctions op by op in
float32, everything else in float64 with a sequential cumsum.  What the device tests compare with, one wall at a time."""
import numpy as np

STATUS_ZERO_LENGTH, STATUS_NON_FINITE = 1, 2
MAX_K = 8


def junction(a, b):
    """(i, j) of the first minimum in row-major order of |a[i] - b[j]|^2; a, b (N, 2) float32; dx*dx + dy*dy, every operation
    rounded to float32 on its own."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(over="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        d = dx * dx + dy * dy
    assert d.dtype == np.float32
    i, j = np.unravel_index(np.argmin(d), d.shape)
    return int(i), int(j)


def runs(junctions, K, N):
    """[(entry, exit)] per contour from the K-1 junctions."""
    if K == 1:
        return [(0, N - 1)]
    out = []
    for k in range(K):
        if k == 0:
            x = junctions[0][0]
            e = 0 if x >= N - 1 - x else N - 1
        else:
            e = junctions[k - 1][1]
            if k == K - 1:
                x = N - 1 if e <= N - 1 - e else 0
            else:
                x = junctions[k][0]
        out.append((e, x))
    return out


def polyline(chain, run_list):
    pieces = []
    for c, (e, x) in zip(chain, run_list):
        idx = np.arange(e, x + 1) if e <= x else np.arange(e, x - 1, -1)
        pieces.append(np.asarray(c, dtype=np.float32)[idx])
    return np.concatenate(pieces).astype(np.float64)


def arc_length(q):
    d = np.diff(q, axis=0)
    seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return np.concatenate([[0.0], np.cumsum(seg)])   # sequential


def resample(q, s, M):
    P, L = len(q), s[-1]
    t = (np.arange(M, dtype=np.float64) * L) / np.float64(M - 1)
    p = np.clip(np.searchsorted(s, t, side="right") - 1, 0, P - 2)
    den = s[p + 1] - s[p]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(den > 0, (t - s[p]) / den, 0.0)
    out = q[p] + f[:, None] * (q[p + 1] - q[p])
    out[0], out[-1] = q[0], q[-1]
    return out


def wall(chain, M):
    """chain (K, N, 2) float32 -> dict: out (M, 2) float64, status, junctions (7, 2) int32 (-1 unused), L, P, q (the polyline)."""
    chain = np.asarray(chain, dtype=np.float32)
    K, N = chain.shape[:2]
    junc = np.full((MAX_K - 1, 2), -1, dtype=np.int32)
    if not np.isfinite(chain).all():
        return dict(out=np.full((M, 2), np.nan), status=STATUS_NON_FINITE, junctions=junc, L=np.nan, P=0, q=None)
    found = [junction(chain[k], chain[k + 1]) for k in range(K - 1)]
    for k, ij in enumerate(found):
        junc[k] = ij
    q = polyline(chain, runs(found, K, N))
    s = arc_length(q)
    if s[-1] == 0:
        return dict(out=np.repeat(q[:1], M, axis=0), status=STATUS_ZERO_LENGTH, junctions=junc, L=0.0, P=len(q), q=q)
    return dict(out=resample(q, s, M), status=0, junctions=junc, L=float(s[-1]), P=len(q), q=q)


def tube(contours, internal, external, M, lengths=None, T=None):
    """contours (F, A, 2, N) float32, internal / external: articulator indices -> air (F, 2, 2, M) float64, status (F, 2),
    junctions (F, 2, 7, 2), length (F, 2), P (F, 2).  Frames f = b T + t with t >= lengths[b] come back as the library's padding."""
    contours = np.asarray(contours, dtype=np.float32)
    F = contours.shape[0]
    air = np.zeros((F, 2, 2, M))
    status = np.zeros((F, 2), dtype=np.int32)
    junc = np.full((F, 2, MAX_K - 1, 2), -1, dtype=np.int32)
    length = np.zeros((F, 2))
    P = np.zeros((F, 2), dtype=np.int64)
    for f in range(F):
        if lengths is not None and f % T >= lengths[f // T]:
            continue
        for w, chain in enumerate((internal, external)):
            r = wall(contours[f, list(chain)].transpose(0, 2, 1), M)
            air[f, w], status[f, w], junc[f, w], length[f, w], P[f, w] = r["out"].T, r["status"], r["junctions"], r["L"], r["P"]
    return air, status, junc, length, P


def bound(P, L):
    """The device's arc lengths differ from the sequential ones in the order of at most P float64 additions, and a lerp carries
    an error in s into the position unamplified: 2 P 2^-53 max(L, 1)."""
    return 2.0 * np.maximum(P, 1) * 2.0 ** -53 * np.maximum(L, 1.0)


# ---------------------------------------------------------------------------------------------------- inputs
def random_chain(rng, K, N, noise=1e-3, reverse=()):
    """An arc of the unit circle cut into K overlapping pieces of N points with radial and tangential noise (uniform in +-noise);
    the pieces whose index is in ``reverse`` are stored backwards.  (K, N, 2) float32."""
    total, overlap = np.pi, 0.25
    span = total / (K - (K - 1) * overlap) if K > 1 else total
    out = []
    for k in range(K):
        a0 = k * span * (1 - overlap)
        ang = np.linspace(a0, a0 + span, N) + rng.uniform(-noise, noise, N)
        rad = 1.0 + rng.uniform(-noise, noise, N)
        c = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
        out.append(c[::-1] if k in reverse else c)
    return np.stack(out).astype(np.float32)


def random_frames(rng, F, A, N, noise=1e-3):
    """(F, A, 2, N) float32: per frame two concentric noisy arcs (radius 1 and 1.5) cut into ceil(A / 2) and floor(A / 2) pieces;
    articulators 0, 2, 4 .. follow the inner arc in order, 1, 3, 5 .. the outer one; about half the pieces stored reversed."""
    out = np.zeros((F, A, 2, N), dtype=np.float32)
    n_in, n_out = (A + 1) // 2, A // 2
    for f in range(F):
        rev = set(np.flatnonzero(rng.random(A) < 0.5).tolist())
        inner = random_chain(rng, n_in, N, noise, {k for k in range(n_in) if 2 * k in rev})
        out[f, 0::2] = inner.transpose(0, 2, 1)
        if n_out:
            outer = 1.5 * random_chain(rng, n_out, N, noise, {k for k in range(n_out) if 2 * k + 1 in rev})
            out[f, 1::2] = outer.transpose(0, 2, 1)
    return out
