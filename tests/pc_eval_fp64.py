"""Float64 yardstick of the principal-components evaluation (NumPy, CPU), written from the definitions: the denormalisation is
x * std + mean in float32 (two rounded operations, what torch computes), the error of a contour pair is the mean over both
directions of the distance from each point to the closest point of the other contour (direct differences, float64) times the
pixel-to-mm factor, and the statistics of a split are the textbook moments of the concatenated rows.  Independent of the library
(no import of artspeech_amd); used by tests/golden/make_golden_pc_eval.py, tests/test_pc_eval_host.py and
tests/test_gpu_pc_eval.py."""
import numpy as np


def denormalise(x, mean, std):
    """x (*lead, A, 2, N) or (*lead, A, 2 N) float32, mean / std (A, 2, N) -> float32 (*lead, A, 2, N)."""
    x = np.asarray(x, np.float32)
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    lead = x.shape[:-2] if x.shape[-1] == 2 * mean.shape[-1] else x.shape[:-3]
    x = x.reshape(*lead, *mean.shape)
    return (x * std).astype(np.float32) + mean


def p2cp_mm(pred, tgt, to_mm=1.0):
    """pred, tgt (*lead, A, 2, N) denormalised -> (*lead, A) float64."""
    p, t = np.asarray(pred, np.float64), np.asarray(tgt, np.float64)
    d = np.sqrt((p[..., 0, :, None] - t[..., 0, None, :]) ** 2 + (p[..., 1, :, None] - t[..., 1, None, :]) ** 2)   # (*, N, N)
    return (d.min(axis=-1).mean(axis=-1) + d.min(axis=-2).mean(axis=-1)) / 2 * to_mm


def shapes_eval(shapes, targets, mean, std, to_mm=1.0, lengths=None, reference=None, ref_idx=-1):
    """as_pc_shapes_eval's three outputs: (pred_out, tgt_out float32 (*lead, A + (ref_idx >= 0), 2, N), p2cp_mm float64
    (*lead, A)); with lengths (B,) the leading shape is (B, T) and the frames t >= lengths[b] are zeros."""
    pred, tgt = denormalise(shapes, mean, std), denormalise(targets, mean, std)
    err = p2cp_mm(pred, tgt, to_mm)
    if ref_idx >= 0:
        ref = np.asarray(reference, np.float32).reshape(*pred.shape[:-3], 1, *pred.shape[-2:])
        pred = np.concatenate([pred[..., :ref_idx, :, :], ref, pred[..., ref_idx:, :, :]], axis=-3)
        tgt = np.concatenate([tgt[..., :ref_idx, :, :], ref, tgt[..., ref_idx:, :, :]], axis=-3)
    if lengths is not None:
        valid = np.arange(pred.shape[1])[None, :] < np.asarray(lengths)[:, None]
        pred, tgt, err = pred * valid[..., None, None, None], tgt * valid[..., None, None, None], err * valid[..., None]
        pred, tgt = pred.astype(np.float32), tgt.astype(np.float32)
    return pred, tgt, err


def moments(x):
    """x (rows, C) -> dict of float64: count, mean (C,), cov (C, C) and std (C,) with n - 1, min, max, median (C,)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    d = x - x.mean(axis=0)
    cov = d.T @ d / (n - 1) if n > 1 else np.full((x.shape[1],) * 2, np.nan)
    return {"count": n, "mean": x.mean(axis=0), "cov": cov, "std": np.sqrt(np.diag(cov)), "min": x.min(axis=0), "max": x.max(axis=0),
            "median": np.median(x, axis=0)}
