"""Float64 yardstick of the result tables of the model-free path (NumPy, CPU), written from the definitions of the reference's
report_phoneme_to_articulation.py: per frame and articulator the point-to-closest-point distance (mean over both directions of
the distance from each point to the closest point of the other contour) and the mean Euclidean distance between corresponding
points, both from direct differences in float64; per articulator mean / std (n - 1) / min / max of those and of their products
with the pixel-to-mm factor; per sentence and tract variable Pearson's r of target and prediction in mm (two passes: means, then
centred sums), NaN for a sentence of fewer than 2 frames or with a constant column (what pandas answers), and mean / std / min /
max of the sentences' coefficients that are not NaN.  Independent of the library (no import of artspeech_amd); used by
tests/golden/make_golden_report.py, tests/test_report_host.py and tests/test_gpu_report.py."""
import numpy as np

TVS = ("LA", "TTCD", "TBCD", "VEL")
METRICS = ("p2cp", "p2cp_mm", "euclidean", "euclidean_mm")
STATS = ("mean", "std", "min", "max")


def frame_metrics(pred, true):
    """pred, true (*lead, A, 2, N) -> (p2cp, euclidean), each float64 (*lead, A)."""
    p, t = np.asarray(pred, np.float64), np.asarray(true, np.float64)
    d = np.sqrt((p[..., 0, :, None] - t[..., 0, None, :]) ** 2 + (p[..., 1, :, None] - t[..., 1, None, :]) ** 2)   # (*, N, N)
    p2cp = (d.min(axis=-1).mean(axis=-1) + d.min(axis=-2).mean(axis=-1)) / 2
    euclid = np.sqrt((p[..., 0, :] - t[..., 0, :]) ** 2 + (p[..., 1, :] - t[..., 1, :]) ** 2).mean(axis=-1)
    return p2cp, euclid


def stats(x):
    """x (n,) without NaN -> [mean, std (n - 1), min, max]; std is NaN below 2 values, everything without one."""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return np.full(4, np.nan)
    mean = x.sum() / x.size
    std = np.sqrt(((x - mean) ** 2).sum() / (x.size - 1)) if x.size > 1 else np.nan
    return np.array([mean, std, x.min(), x.max()])


def segment_corr(a, b, seg_first, scale=1.0):
    """a, b (rows, K), seg_first (S + 1,) -> corr (S, K), summary (5, K) = count | mean | std | min | max of the corr that are
    not NaN.  Every value is x * scale in float64."""
    a, b = np.asarray(a, np.float64) * scale, np.asarray(b, np.float64) * scale
    seg_first = np.asarray(seg_first, np.int64)
    S, K = len(seg_first) - 1, a.shape[1]
    corr = np.full((S, K), np.nan)
    for s in range(S):
        r0, r1 = max(int(seg_first[s]), 0), min(int(seg_first[s + 1]), a.shape[0])
        if r1 - r0 < 2:
            continue
        for k in range(K):
            x, y = a[r0:r1, k], b[r0:r1, k]
            if (x == x[0]).all() or (y == y[0]).all():
                continue
            xc, yc = x - x.sum() / x.size, y - y.sum() / y.size
            corr[s, k] = (xc * yc).sum() / np.sqrt((xc * xc).sum() * (yc * yc).sum())
    summary = np.full((5, K), np.nan)
    for k in range(K):
        c = corr[:, k][np.isfinite(corr[:, k])]
        summary[0, k] = c.size
        summary[1:, k] = stats(c)
    return corr, summary


def frame_order(sentences, frames):
    """The reference's row order: sentences by name, the frames of a sentence by integer value.  Returns (order (rows,) into
    the given lists, names (S,) sorted, seg_first (S + 1,) into the ordered rows)."""
    keys = sorted(range(len(sentences)), key=lambda i: (str(sentences[i]), int(frames[i])))
    names = sorted(set(str(s) for s in sentences))
    counts = [sum(1 for s in sentences if str(s) == n) for n in names]
    return np.array(keys, np.int64), names, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def report(sentences, frames, phonemes, pred, true, tv_pred, tv_target, articulators, to_mm):
    """The three tables from per-frame inputs in any order: sentences / frames / phonemes (rows,), pred / true
    (rows, A, 2, N) with the channels in the order of `articulators`, tv_pred / tv_target (rows, 4) in pixels.
      full   {"sentence_name", "frame" (int), "phoneme", "articulator": lists of rows * A entries, sentence -> frame ->
             articulator; "values": (rows * A, 4) in METRICS order}
      agg    {"articulator": sorted names, "values": (A, 16): METRICS x STATS}
      corr   (S, 4) per sorted sentence and TV;  corr_report (4, 4): TVS x STATS"""
    order, names, seg_first = frame_order(sentences, frames)
    A = len(articulators)
    p2cp, euclid = frame_metrics(np.asarray(pred)[order], np.asarray(true)[order])
    values = np.stack([p2cp, p2cp * to_mm, euclid, euclid * to_mm], axis=-1)          # (rows, A, 4)
    full = {"sentence_name": [str(sentences[i]) for i in order for _ in range(A)],
            "frame": [int(frames[i]) for i in order for _ in range(A)],
            "phoneme": [str(phonemes[i]) for i in order for _ in range(A)],
            "articulator": [a for _ in order for a in articulators],
            "values": values.reshape(-1, 4)}
    by_name = sorted(range(A), key=lambda i: articulators[i])
    agg = {"articulator": [articulators[i] for i in by_name],
           "values": np.stack([np.concatenate([stats(values[:, i, m]) for m in range(4)]) for i in by_name])}
    corr, summary = segment_corr(np.asarray(tv_target, np.float64)[order], np.asarray(tv_pred, np.float64)[order], seg_first, to_mm)
    return {"full": full, "agg": agg, "corr": corr, "corr_report": summary[1:].T.copy(), "sentences": names}
