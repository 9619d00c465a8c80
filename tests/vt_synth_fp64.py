"""The numpy restatement of the speech synthesis from the tube (artspeech_amd/csrc/vt_synth.hip: as_vt_glottal_source,
as_vt_waveguide; artspeech_amd/vocal_tract_synthesis.py: equal_sections, frication_control), written from the definition in
include/artspeech_hip.h, in float64 or -- ``dtype=np.longdouble`` -- in the widest float the machine has.  The ladder is
vectorised over the batch and walks the samples in a Python loop.  ``CASES`` and ``draw_case`` are the shapes the device tests run."""
import numpy as np

MIN_AREA = 1e-4
RISE, FALL = 0.40, 0.16
R_GLOTTIS, R_LIPS, MU = 0.75, -0.85, 0.999
SOUND_SPEED = 35000.0
_M64 = (1 << 64) - 1


def noise(seed, stream, b, n):
    """nu(seed, stream, b, n) in [-1, 1) for an array n of sample indices: float64, exact."""
    n = np.asarray(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        idx = np.uint64(((2 * int(b) + int(stream)) << 40) & _M64) | n
        z = np.uint64(int(seed) & _M64) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return 2.0 * u - 1.0


def pulse(theta, rise=RISE, fall=FALL):
    """The Rosenberg pulse at theta in [0, 1), in theta's dtype."""
    theta = np.asarray(theta)
    dt = theta.dtype.type
    pi = dt(np.pi) if dt is np.float64 else np.arctan(dt(1)) * 4
    up = (1 - np.cos(pi * theta / dt(rise))) / 2
    down = np.cos(pi * (theta - dt(rise)) / (2 * dt(fall)))
    return np.where(theta < dt(rise), up, np.where(theta < dt(rise) + dt(fall), down, dt(0)))


def _interp(x, F, S, dtype):
    """A per-frame control (F values used) at its F S samples: x_t + (x_t' - x_t) (s / S), t' = min(t + 1, F - 1)."""
    x = np.asarray(x[:F], dtype)
    nxt = x[np.minimum(np.arange(F) + 1, F - 1)]
    frac = np.arange(S, dtype=dtype) / dtype(S)
    return (x[:, None] + (nxt - x)[:, None] * frac[None, :]).reshape(-1)


def phase(f0, F, S, fs, dtype=np.float64):
    """The phase in cycles at every sample of one utterance, by the closed form: base_t + (g_t s + d_t (s (s - 1) / 2) / S) / fs."""
    g = np.maximum(np.asarray(f0[:F], dtype), 0)
    d = g[np.minimum(np.arange(F) + 1, F - 1)] - g
    total = (g * dtype(S) + d * ((dtype(S) - 1) / 2)) / dtype(fs)
    base = np.concatenate([[dtype(0)], np.cumsum(total)[:-1]]) if F else np.zeros(0, dtype)
    s = np.arange(S, dtype=dtype)
    within = g[:, None] * s[None, :] + d[:, None] * ((s * (s - 1) / 2) / dtype(S))[None, :]
    return (base[:, None] + within / dtype(fs)).reshape(-1)


def phase_running_sum(f0, F, S, fs, dtype=np.longdouble):
    """The same phase as the plain running sum of its definition: sum_{m < n} g[m] / fs."""
    g = _interp(np.maximum(np.asarray(f0, dtype), 0), F, S, dtype)
    return np.concatenate([[dtype(0)], np.cumsum(g / dtype(fs))[:-1]]) if F else np.zeros(0, dtype)


def source(f0, voiced, asp, frames, S, fs, seed=0, rise=RISE, fall=FALL, dtype=np.float64, pitch=None):
    """as_vt_glottal_source: (source (B, pitch), status (B,), cycles (B,) the total phase of each row)."""
    f0, voiced, asp = (np.asarray(x, np.float64) for x in (f0, voiced, asp))
    B, T = f0.shape
    pitch = T * S if pitch is None else pitch
    out = np.zeros((B, pitch), dtype)
    status = np.zeros(B, np.int32)
    cycles = np.zeros(B)
    for b in range(B):
        F = int(np.clip(frames[b], 0, T))
        n = F * S
        if not (np.isfinite(f0[b, :F]).all() and np.isfinite(voiced[b, :F]).all() and np.isfinite(asp[b, :F]).all()):
            status[b] = 2
            out[b, :n] = np.nan
            continue
        if n == 0:
            continue
        ph = phase(f0[b], F, S, fs, dtype)
        cycles[b] = float(ph[-1])
        theta = ph - np.floor(ph)
        nu = noise(seed, 0, b, np.arange(n)).astype(dtype)
        out[b, :n] = _interp(voiced[b], F, S, dtype) * pulse(theta, rise, fall) + _interp(asp[b], F, S, dtype) * nu
    return out, status, cycles


def ladder(areas, sections, frames, S, src, inject_section=None, inject_gain=None, seed=0, r_g=R_GLOTTIS, r_l=R_LIPS, mu=MU,
           min_area=MIN_AREA, radiation=1, dtype=np.float64):
    """as_vt_waveguide: (out (B, pitch) in ``dtype``, status (B,)).  areas (B, T, Kmax), src (B, pitch) float64."""
    areas = np.asarray(areas, np.float64)
    src64 = np.asarray(src, np.float64)
    B, T, Kmax = areas.shape
    pitch = src64.shape[1]
    sections = np.asarray(sections, np.int64)
    F = np.clip(np.asarray(frames, np.int64), 0, T)
    nb = F * S
    out = np.zeros((B, pitch), dtype)
    status = np.zeros(B, np.int32)
    j = np.arange(Kmax)
    gain64 = None if inject_gain is None else np.asarray(inject_gain, np.float64)
    for b in range(B):
        a = areas[b, :F[b], :sections[b]]
        bad = not (np.isfinite(a).all() and (a > 0).all() and np.isfinite(src64[b, :nb[b]]).all())
        if gain64 is not None:
            bad = bad or not np.isfinite(gain64[b, :F[b]]).all()
        if bad:
            status[b] |= 2
            out[b, :nb[b]] = np.nan
        elif (a < min_area).any():
            status[b] |= 1
    live = (status & 2) == 0
    # reflection coefficients per frame, zero where an utterance has no junction
    with np.errstate(all="ignore"):
        A = np.maximum(np.where(np.isfinite(areas), areas, 1.0), min_area).astype(dtype)
        kf = (A[:, :, :-1] - A[:, :, 1:]) / (A[:, :, :-1] + A[:, :, 1:])
    kf = np.where(j[None, None, :-1] < (sections - 1)[:, None, None], kf, dtype(0))
    R = np.zeros((B, Kmax), dtype)
    L = np.zeros((B, Kmax), dtype)
    y_prev = np.zeros(B, dtype)
    rows = np.arange(B)
    lips = sections - 1
    r_g, r_l, mu = dtype(r_g), dtype(r_l), dtype(mu)
    n_max = int(nb[live].max()) if live.any() else 0
    if inject_section is not None:
        nu = np.stack([noise(seed, 1, b, np.arange(n_max)) for b in range(B)]).astype(dtype).reshape(B, n_max)
    for n in range(n_max):
        t_raw, s = divmod(n, S)
        run = live & (n < nb)
        t = np.minimum(t_raw, np.maximum(F - 1, 0))
        tn = np.minimum(t + 1, np.maximum(F - 1, 0))
        frac = dtype(s) / dtype(S)
        y = (1 + r_l) * R[rows, lips]
        o = y - y_prev if radiation else y
        y_prev = y
        out[run, n] = o[run]
        k0 = kf[rows, t] if Kmax > 1 else np.zeros((B, 0), dtype)
        k = k0 + (kf[rows, tn] - k0) * frac if Kmax > 1 else k0
        w = k * (R[:, :-1] - L[:, 1:])
        Rn = np.empty_like(R)
        Ln = np.zeros_like(L)
        Rn[:, 1:] = R[:, :-1] + w
        if inject_section is not None:
            sec = np.asarray(inject_section)[rows, t]
            g0 = gain64[rows, t].astype(dtype)
            g = g0 + (gain64[rows, tn].astype(dtype) - g0) * frac
            e = g * nu[:, n]
            hit = (sec >= 0) & run
            with np.errstate(invalid="ignore"):
                Rn[rows[hit], sec[hit]] += e[hit]
        Rn[:, 1:] *= mu
        Ln[:, :-1] = mu * (L[:, 1:] + w)
        Rn[:, 0] = mu * (src64[:, min(n, pitch - 1)].astype(dtype) + r_g * L[:, 0])
        Ln[rows, lips] = mu * (r_l * R[rows, lips])
        R = np.where(run[:, None], Rn, R)
        L = np.where(run[:, None], Ln, L)
    return out, status


def equal_sections(areas, lengths, counts, frames, fs, c=SOUND_SPEED):
    """vocal_tract_synthesis.equal_sections, frame by frame: (areas_eq (B, T, Kmax), sections (B,), tract_length (B, 3), replaced (B,))."""
    areas, lengths = np.asarray(areas, np.float64), np.asarray(lengths, np.float64)
    B, T, Kr = areas.shape
    sections, stats, replaced, rows = [], [], [], []
    for b in range(B):
        F = int(np.clip(frames[b], 0, T))
        cnt = np.minimum(np.asarray(counts[b], np.int64), Kr)
        valid = [t < F and cnt[t] >= 1 and bool(np.isfinite(areas[b, t, :cnt[t]]).all() and np.isfinite(lengths[b, t, :cnt[t]]).all()
                                                  and (lengths[b, t, :cnt[t]] > 0).all()) for t in range(T)]
        total = [float(np.cumsum(lengths[b, t, :max(cnt[t], 0)])[-1]) if cnt[t] >= 1 else 0.0 for t in range(T)]
        good = [total[t] for t in range(T) if valid[t]]
        mean = sum(good) / len(good) if good else float("nan")
        K = int(np.clip(np.round((mean if good else 0.0) * fs / c), 2, 64))
        sections.append(K)
        stats.append([min(good), mean, max(good)] if good else [np.nan] * 3)
        replaced.append(sum(1 for t in range(F) if not valid[t]))
        per_frame = []
        for t in range(T):
            if not valid[t]:
                per_frame.append(None)
                continue
            ends = np.cumsum(lengths[b, t, :cnt[t]])
            mid = (np.arange(K) + 0.5) * (total[t] / K)
            per_frame.append(areas[b, t, np.minimum(np.searchsorted(ends, mid, side="right"), cnt[t] - 1)])
        first = next((t for t in range(T) if valid[t]), None)
        filled, last = [], None
        for t in range(T):
            last = t if valid[t] else last
            src = last if last is not None else first
            filled.append(np.full(K, np.nan) if src is None else per_frame[src])
            if t >= F:
                filled[-1] = np.zeros(K)
        rows.append(filled)
    Kmax = max(sections) if B else 2
    out = np.zeros((B, T, Kmax))
    for b in range(B):
        for t in range(T):
            out[b, t, :sections[b]] = rows[b][t]
    return out, np.array(sections, np.int32), np.array(stats).reshape(B, 3), np.array(replaced, np.int64)


def frication_control(areas_eq, sections, gain, critical_area=0.2, min_area=MIN_AREA):
    """vocal_tract_synthesis.frication_control: (inject_section (B, T) int32, inject_gain (B, T))."""
    areas_eq = np.asarray(areas_eq, np.float64)
    B, T, _ = areas_eq.shape
    gain = np.broadcast_to(np.asarray(gain, np.float64), (B, T))
    where = np.full((B, T), -1, np.int32)
    q = np.zeros((B, T))
    for b in range(B):
        K = int(sections[b])
        for t in range(T):
            inner = areas_eq[b, t, 1:K - 1]
            inner = np.where(np.isnan(inner), np.inf, inner)
            if inner.size == 0 or not np.isfinite(inner.min()) or inner.min() < min_area:
                continue
            m = 1 + int(np.argmin(inner))
            value = gain[b, t] * max(0.0, 1.0 - inner.min() / critical_area)
            if value > 0:
                where[b, t], q[b, t] = min(m + 1, K - 1), value
    return where, q


def steady_state(areas, omega, r_g, r_l, mu):
    """The static ladder's response y / source at z = exp(j omega) by a direct solve of its 2K steady-state equations (no
    differencing): the unknowns are R_0 .. R_{K-1}, L_0 .. L_{K-1}, and z X = M X + mu e_0."""
    A = np.asarray(areas, np.float64)
    K = len(A)
    k = (A[:-1] - A[1:]) / (A[:-1] + A[1:])
    M = np.zeros((2 * K, 2 * K))
    for j in range(K - 1):
        M[j + 1, j] += mu * (1 + k[j])          # R'_{j+1} = mu (R_j + k_j (R_j - L_{j+1}))
        M[j + 1, K + j + 1] += -mu * k[j]
        M[K + j, K + j + 1] += mu * (1 - k[j])  # L'_j = mu (L_{j+1} + k_j (R_j - L_{j+1}))
        M[K + j, j] += mu * k[j]
    M[0, K] = mu * r_g
    M[2 * K - 1, K - 1] = mu * r_l
    rhs = np.zeros(2 * K, complex)
    rhs[0] = mu
    out = np.empty(len(omega), complex)
    for i, w in enumerate(omega):
        x = np.linalg.solve(np.exp(1j * w) * np.eye(2 * K) - M, rhs)
        out[i] = (1 + r_l) * x[K - 1]
    return out


# (B, T, S, sections per utterance, frames per utterance, radiation, injection) -- the smallest shapes at which the kernel can go
# wrong: K at the lane, DPP-row and wave ends, S around the 64-sample batches, one frame, ragged frames with 0, ragged sections.
CASES = [
    (3, 9, 64, (1, 2, 64), (9, 9, 9), 1, False),
    (4, 9, 65, (16, 17, 32, 33), (9, 5, 0, 1), 1, True),
    (2, 9, 63, (63, 64), (9, 8), 0, True),
    (5, 2, 1, (1, 2, 17, 33, 64), (2, 1, 2, 0, 2), 1, True),
    (3, 9, 2, (2, 16, 63), (9, 2, 7), 0, True),
    (2, 1, 65, (32, 3), (1, 1), 1, True),
    (1, 9, 500, (22,), (9,), 1, True),
]
CASE_IDS = ["B{}-T{}-S{}-K{}-rad{}-{}".format(c[0], c[1], c[2], "_".join(map(str, c[3])), c[5], "inj" if c[6] else "plain") for c in CASES]


def draw_case(case, seed=0):
    """The seeded inputs of one of CASES: areas exp(N(0, 0.7)) that drift from frame to frame, a pulse-and-noise source of a
    few hundred Hz from the restated source itself, injection at section 1, at K - 1 and nowhere in turn."""
    B, T, S, sections, frames, radiation, inject = case
    rng = np.random.default_rng([seed, B, T, S, sum(sections)])
    Kmax = max(sections)
    areas = np.exp(0.7 * rng.standard_normal((B, 1, Kmax)) + 0.4 * rng.standard_normal((B, T, Kmax)))
    fs = 50.0 * S if S >= 64 else 3200.0
    f0 = rng.uniform(90.0, 320.0, (B, T))
    src, _, _ = source(f0, rng.uniform(0.5, 1.0, (B, T)), rng.uniform(0.0, 0.2, (B, T)), frames, S, fs, seed=seed + 5)
    where = gain = None
    if inject:
        where = np.full((B, T), -1, np.int32)
        for b in range(B):
            K = sections[b]
            if K >= 2:
                choice = [1, K - 1, -1, min(2, K - 1)]
                where[b] = [choice[(t + b) % 4] for t in range(T)]
        gain = rng.uniform(0.0, 0.3, (B, T))
    return dict(areas=areas, sections=np.array(sections, np.int32), frames=np.array(frames, np.int32), S=S, source=src, where=where,
                gain=gain, seed=seed + 11, radiation=radiation, fs=fs, f0=f0)
