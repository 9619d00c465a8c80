"""Restatement of the contour preparation in index arithmetic (numpy, float32, no device): what csrc/contours.hip computes,
written the way the kernel thinks about it -- kept sets and ``(j * n) // 50`` -- and held to the reference's own outputs bit for
bit by tests/test_contours_host.py.  Yardstick of the GPU tests for the shapes the fixture does not hold."""
import numpy as np

POINTS = 50
HALF = 25
KINDS = {"tongue": 1, "lower-lip": 2, "upper-lip": 3}
REFERENCES = ["lower-incisor", "upper-incisor", "epiglottis"]


def thresholds(dataset_config):
    """the four margins, each computed in double and rounded once to float32"""
    spacing, res = dataset_config.PIXEL_SPACING, dataset_config.RES
    return tuple(np.float32(v) for v in (10 / spacing / res, 5 / spacing / res, 10 / spacing, 5 / spacing))


def nearest_index(n, size=POINTS):
    """source indices of F.interpolate(size=size) in nearest mode over n points"""
    return (np.arange(size) * n) // size


def kinds_of(articulators, clip_tails=True):
    return [KINDS.get(a, 0) if clip_tails else 0 for a in articulators]


def clip(kind, points, lower_incisor, upper_incisor, epiglottis, thr):
    """points (50, 2) float32 -> (clipped (50, 2), points kept before the last resampling); count 0: a NaN contour"""
    points = np.asarray(points, np.float32)
    if kind == 0:
        return points.copy(), len(points)
    assert points.shape == (POINTS, 2)
    y = points[:, 1]
    first = np.arange(POINTS) < HALF
    if kind == 1:
        li_max, ep_min = np.float32(lower_incisor[:, 1].max()), np.float32(epiglottis[:, 1].min())
        keep = np.where(first, y < np.float32(ep_min + thr[0]), y < li_max)
    elif kind == 3:
        ry = np.float32(upper_incisor[-1, 1])
        keep = np.where(first, y > np.float32(ry - thr[3]), y > np.float32(ry - thr[2]))
    else:
        li_max = np.float32(lower_incisor[:, 1].max())
        keep = first | (y < np.float32(li_max + thr[1]))
        points = points[np.flatnonzero(keep)[nearest_index(int(keep.sum()))]]
        keep = ~first | (points[:, 1] < li_max)
    n = int(keep.sum())
    if n == 0:
        return np.full((POINTS, 2), np.nan, np.float32), 0
    return points[np.flatnonzero(keep)[nearest_index(n)]], n


def clip_batched(raw, refs, kinds, thr):
    """raw (F, A, 50, 2), refs (F, 3, 50, 2) -> clipped (F, A, 50, 2), counts int32 (F, A)"""
    raw = np.asarray(raw, np.float32)
    out = np.empty_like(raw)
    counts = np.empty(raw.shape[:2], np.int32)
    for f in range(raw.shape[0]):
        for a, kind in enumerate(kinds):
            out[f, a], counts[f, a] = clip(kind, raw[f, a], refs[f, 0], refs[f, 1], refs[f, 2], thr)
    return out, counts


def prepare(raw, refs, kinds, thr, mean=None, std=None):
    """-> targets (F, A, 2, N), references (F, 1, 2, N), counts (F, A): clipped, (p - u) + 0.3 with u the last point of the raw
    upper incisor (two float32 operations), then (x - mean) / std with mean, std (A, 2, N)"""
    raw, refs = np.asarray(raw, np.float32), np.asarray(refs, np.float32)
    clipped, counts = clip_batched(raw, refs, kinds, thr) if any(kinds) else (raw, np.full(raw.shape[:2], raw.shape[2], np.int32))
    u = refs[:, 1, -1, :][:, None, :, None]                                      # (F, 1, 2, 1)
    targets = (clipped.transpose(0, 1, 3, 2) - u) + np.float32(0.3)
    references = (refs[:, 1:2].transpose(0, 1, 3, 2) - u) + np.float32(0.3)
    if mean is not None:
        targets = (targets - np.asarray(mean, np.float32)[None]) / np.asarray(std, np.float32)[None]
    return targets.astype(np.float32), references.astype(np.float32), counts


def column_stats_fp64(x):
    """mean and unbiased std over axis 0 in fp64 (two passes); one row: NaN std"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((x - mean) ** 2).sum(axis=0) / np.float64(x.shape[0] - 1)) if x.shape[0] > 1 else np.full(x.shape[1:], np.nan)
    return mean, std
