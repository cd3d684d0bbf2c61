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


class StrataSpec:
    """How the device evaluation splits the counted pixels of an image (include/gedepth_strata.h): ``edges``, up to seven finite, strictly
    ascending distances in metres, cut the ground truth into ``len(edges) + 1`` bins (a ground truth on an edge belongs to the upper bin);
    ``ground`` splits every bin into the returns off and on the ground plane the front end was fed, on meaning
    ``g > 0 and |gt - g| <= ground_tol * g``.  ``ground_tol`` in [0, 1] is the caller's choice, not a measured constant."""

    def __init__(self, edges=(20, 40, 60), ground=True, ground_tol=0.1):
        self.edges = tuple(float(e) for e in edges)
        self.ground, self.ground_tol = bool(ground), float(ground_tol)
        if len(self.edges) > 7:
            raise ValueError(f'StrataSpec takes 0 .. 7 bin edges, got {len(self.edges)}')
        if any(not np.isfinite(e) for e in self.edges) or any(b <= a for a, b in zip(self.edges, self.edges[1:])):
            raise ValueError(f'StrataSpec: bin edges must be finite and strictly ascending, got {self.edges}')
        if not 0.0 <= self.ground_tol <= 1.0:
            raise ValueError(f'StrataSpec: ground_tol must lie in [0, 1], got {ground_tol}')

    @property
    def count(self):
        """S, the number of strata."""
        return (len(self.edges) + 1) * (2 if self.ground else 1)

    def names(self, min_depth=1e-3, max_depth=80):
        """The S stratum names, bin-major: '0-20m/other', '0-20m/ground', ..., '60-80m/ground'; without ``ground`` the bin alone.  The first
        bin starts at ``min_depth`` (written 0 below 1 m) and the last ends at ``max_depth``."""
        bounds = ['0' if min_depth < 1 else f'{float(min_depth):g}'] + [f'{e:g}' for e in self.edges] + [f'{float(max_depth):g}']
        bins = [f'{lo}-{hi}m' for lo, hi in zip(bounds, bounds[1:])]
        if not self.ground:
            return bins
        return [f'{b}/{c}' for b in bins for c in ('other', 'ground')]

    def __repr__(self):
        return f'StrataSpec(edges={self.edges}, ground={self.ground}, ground_tol={self.ground_tol})'


def strata_table(rows, spec, min_depth=1e-3, max_depth=80):
    """``rows`` (N, S, 10) float64, every image's metric sums per stratum -> OrderedDict stratum name -> OrderedDict of the nine metrics
    plus ``pixels`` (the stratum's share of all counted pixels) and ``images`` (the number of images where it is non-empty).  A stratum's
    metric is the nan-mean over images of ``metrics_from_sums(row)``, the convention of the headline numbers: an image where the stratum
    is empty is skipped, a stratum that is empty everywhere is all-NaN."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[1:] != (spec.count, 10):
        raise ValueError(f'rows must be (N, {spec.count}, 10), got {rows.shape}')
    total = rows[:, :, 0].sum()
    table = OrderedDict()
    for s, name in enumerate(spec.names(min_depth, max_depth)):
        filled = [metrics_from_sums(r) for r in rows[:, s] if r[0] > 0]
        entry = OrderedDict((m, float(np.mean([t[k] for t in filled])) if filled else np.nan) for k, m in enumerate(METRIC_NAMES))
        entry['pixels'] = float(rows[:, s, 0].sum() / total) if total > 0 else np.nan
        entry['images'] = len(filled)
        table[name] = entry
    return table
