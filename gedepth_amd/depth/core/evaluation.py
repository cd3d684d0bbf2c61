"""Depth metrics of the evaluation protocol (mirror of depth/core/evaluation/metrics.py:8-100).
Host-side numpy on per-image arrays, exactly as the reference evaluates them (nan-mean over images)."""
from collections import OrderedDict

import numpy as np

METRIC_NAMES = ('a1', 'a2', 'a3', 'abs_rel', 'rmse', 'log_10', 'rmse_log', 'silog', 'sq_rel')


def calculate(gt, pred):
    if gt.shape[0] == 0:
        return (np.nan,) * 9
    ratio = np.maximum(gt / pred, pred / gt)
    a1, a2, a3 = [(ratio < 1.25 ** p).mean() for p in (1, 2, 3)]
    diff = gt - pred
    abs_rel = np.mean(np.abs(diff) / gt)
    sq_rel = np.mean(diff ** 2 / gt)
    rmse = np.sqrt(np.mean(diff ** 2))
    log_diff = np.log(pred) - np.log(gt)
    rmse_log = np.sqrt(np.mean(log_diff ** 2))
    silog = np.sqrt(np.mean(log_diff ** 2) - np.mean(log_diff) ** 2) * 100
    if np.isnan(silog):
        silog = 0
    log_10 = np.mean(np.abs(np.log10(gt) - np.log10(pred)))
    return a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel


def metrics(gt, pred, min_depth=1e-3, max_depth=80):
    mask = np.logical_and(gt > min_depth, gt < max_depth)
    return calculate(gt[mask], pred[mask])


def eval_metrics(gt, pred, min_depth=1e-3, max_depth=80):
    return dict(zip(METRIC_NAMES, metrics(gt, pred, min_depth, max_depth)))


def metrics_from_sums(sums):
    """One image's ten float64 sums of ``kernels.depth_metric_sums`` (n, the three threshold counts, sum |d| / gt, sum d^2 / gt, sum d^2,
    sum l, sum l^2, sum |log10 gt - log10 pred|; d = gt - pred, l = log pred - log gt) -> the tuple ``calculate`` returns."""
    n, c1, c2, c3, s_abs, s_sq, s_d2, s_l, s_l2, s_l10 = (float(v) for v in sums)
    if n == 0:
        return (np.nan,) * 9
    with np.errstate(invalid='ignore'):
        mean_l2 = np.float64(s_l2) / n
        rmse_log = np.sqrt(mean_l2)
        silog = np.sqrt(mean_l2 - (np.float64(s_l) / n) ** 2) * 100
    if np.isnan(silog):
        silog = 0
    return c1 / n, c2 / n, c3 / n, s_abs / n, np.sqrt(np.float64(s_d2) / n), s_l10 / n, rmse_log, silog, s_sq / n


def pre_eval_to_metrics(pre_eval_results):
    cols = tuple(zip(*pre_eval_results))
    return OrderedDict((name, np.nanmean(cols[i])) for i, name in enumerate(METRIC_NAMES))
