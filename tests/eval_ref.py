"""float64 restatement of depth/core/evaluation.py ``calculate`` for the device-evaluation tests (imported like ``f64ref``).

The three threshold tests are discontinuous, so they stay what ``calculate`` does: float32 divisions, ``np.maximum``, a comparison with
``1.25 ** p``.  Everything continuous is formed in float64 from the float32 inputs."""
import numpy as np

SUM_NAMES = ('n', 'c1', 'c2', 'c3', 'abs_rel', 'sq_rel', 'd2', 'l', 'l2', 'log10')
LOG_SUMS = (7, 8, 9)                      # the sums that contain a logarithm


def sums_f64(gt, pred):
    """The ten sums of ``ge_depth_metrics`` over the 1-D float32 arrays of the pixels that count."""
    gt, pred = np.asarray(gt, np.float32), np.asarray(pred, np.float32)
    with np.errstate(all='ignore'):
        ratio = np.maximum(gt / pred, pred / gt)
        counts = [float((ratio < 1.25 ** p).sum()) for p in (1, 2, 3)]
        g, q = gt.astype(np.float64), pred.astype(np.float64)
        d = g - q
        l = np.log(q) - np.log(g)
        return np.array([float(gt.size)] + counts + [(np.abs(d) / g).sum(), (d * d / g).sum(), (d * d).sum(), l.sum(), (l * l).sum(),
                                                      np.abs(np.log10(g) - np.log10(q)).sum()], np.float64)


def calculate_f64(gt, pred):
    """``calculate`` with every continuous term in float64 (the same order of operations, means by ``np.mean``)."""
    gt, pred = np.asarray(gt, np.float32), np.asarray(pred, np.float32)
    if gt.shape[0] == 0:
        return (np.nan,) * 9
    with np.errstate(all='ignore'):
        ratio = np.maximum(gt / pred, pred / gt)
        a1, a2, a3 = [(ratio < 1.25 ** p).mean() for p in (1, 2, 3)]
        g, q = gt.astype(np.float64), pred.astype(np.float64)
        diff = g - q
        abs_rel = np.mean(np.abs(diff) / g)
        sq_rel = np.mean(diff ** 2 / g)
        rmse = np.sqrt(np.mean(diff ** 2))
        log_diff = np.log(q) - np.log(g)
        rmse_log = np.sqrt(np.mean(log_diff ** 2))
        silog = np.sqrt(np.mean(log_diff ** 2) - np.mean(log_diff) ** 2) * 100
        if np.isnan(silog):
            silog = 0
        log_10 = np.mean(np.abs(np.log10(g) - np.log10(q)))
    return a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel


def window(gt_raw, top, left, Hc, Wc, depth_scale=256):
    """``KITTIDataset._gt`` followed by the crop: float32 division of the raw PNG values."""
    return (np.asarray(gt_raw, dtype=np.float32) / depth_scale)[top:top + Hc, left:left + Wc]


def mask_of(gt, rect, min_depth=1e-3, max_depth=80):
    """``eval_mask`` for a rectangle (r0, r1, c0, c1)."""
    valid = np.logical_and(gt > min_depth, gt < max_depth)
    crop = np.zeros(valid.shape, bool)
    crop[rect[0]:rect[1], rect[2]:rect[3]] = True
    return np.logical_and(valid, crop)
