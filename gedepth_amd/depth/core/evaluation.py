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


class PriorSweep:
    """Which ground priors ``single_gpu_test(..., device_eval=True, prior_sweep=PriorSweep(...))`` evaluates every frame under
    (include/gedepth_sweep.h states the rule): the baseline — the calibrated plane, untouched — first, then one variant per entry of
    ``pitch_deg`` (degrees; positive: the ground comes closer, as when the camera pitches down against its calibration), then one per entry
    of ``height_scale`` (the plane of a camera that many times as high), then, with ``drop``, the prior removed (all zeros).  At most eight
    variants: they are the slots of one forward.  ``cam_height`` (metres) turns a pitch into the rule's ``c = tan(pitch) / cam_height``,
    formed in float64 and rounded to float32 once.  ``variants``: the ``(c, s, drop)`` rows, ``names`` their labels, ``count`` their number."""

    MAX = 8                            # GE_SWEEP_MAX of include/gedepth_sweep.h

    def __init__(self, pitch_deg=(-1.0, -0.5, 0.5, 1.0), height_scale=(), drop=True, cam_height=1.65):
        self.pitch_deg = tuple(float(d) for d in pitch_deg)
        self.height_scale = tuple(float(s) for s in height_scale)
        self.drop, self.cam_height = bool(drop), float(cam_height)
        if not (np.isfinite(self.cam_height) and self.cam_height > 0.0):
            raise ValueError(f'PriorSweep: cam_height must be a positive number of metres, got {cam_height}')
        for d in self.pitch_deg:
            if not np.isfinite(d) or abs(d) > 10.0 or d == 0.0:
                raise ValueError(f'PriorSweep: a pitch must be finite, within +-10 degrees and not 0 (the baseline is always the first '
                                 f'variant), got {d}')
        for s in self.height_scale:
            if not np.isfinite(s) or not 0.5 <= s <= 2.0 or s == 1.0:
                raise ValueError(f'PriorSweep: a height scale must lie in [0.5, 2] and not be 1 (the baseline is always the first variant), '
                                 f'got {s}')
        self.variants = [(0.0, 1.0, 0)]
        self.names = ['baseline']
        for d in self.pitch_deg:
            self.variants.append((float(np.float32(np.tan(np.radians(d)) / self.cam_height)), 1.0, 0))
            self.names.append(f'pitch {d:+.2f} deg')
        for s in self.height_scale:
            self.variants.append((0.0, float(np.float32(s)), 0))
            self.names.append(f'height x{s:.2f}')
        if self.drop:
            self.variants.append((0.0, 1.0, 1))
            self.names.append('no prior')
        if len(self.variants) > self.MAX:
            raise ValueError(f'PriorSweep: at most {self.MAX} variants (the slots of one forward), the baseline included, got {len(self.variants)}')
        if len(set(self.variants)) != len(self.variants) or len(set(self.names)) != len(self.names):
            raise ValueError(f'PriorSweep: duplicate variants in pitch_deg={self.pitch_deg}, height_scale={self.height_scale}')

    @property
    def count(self):
        """V, the number of variants."""
        return len(self.variants)

    def table(self):
        """The ``(c, s, drop)`` rows as the ``GePriorVariant`` struct of include/gedepth_sweep.h takes them: two float32 values as Python
        floats and an int."""
        return list(self.variants)

    def __repr__(self):
        return f'PriorSweep(pitch_deg={self.pitch_deg}, height_scale={self.height_scale}, drop={self.drop}, cam_height={self.cam_height})'


class ErrorMaps:
    """Where in the picture a split's error is (include/gedepth_error.h), for ``single_gpu_test(..., device_eval=True, errors=ErrorMaps(...))``:
    the loop adds every LiDAR return's abs-rel error e = |gt - pred| / gt into a per-pixel float64 ``sum`` and uint32 ``count`` on the
    device (a NaN or infinite e enters neither) and, with ``out_dir``, writes one error picture per image there.  After the loop ``sum``
    and ``count`` are (352, 1216) numpy planes, ``frames`` the number of images, ``rect`` the dataset's evaluation rectangle.

    ``tau`` in (0, 1]: the abs-rel error at the middle threshold of the ten colour bands (0.05: red from 5 %); ``radius`` 0 .. 3: a return
    is drawn (2 radius + 1) pixels wide, the worst one winning; ``background``: 0 the frame, 1 the frame halved, 2 black.  They are the
    caller's choices, not measured constants."""

    def __init__(self, out_dir=None, tau=0.05, radius=1, background=1):
        if out_dir is not None and not isinstance(out_dir, str):
            raise TypeError(f'ErrorMaps: out_dir must be a directory path or None, got {out_dir!r}')
        from ...error_kernels import paint_args                        # the one statement of the three ranges (the module loads no library)
        self.tau, self.radius, self.background = paint_args(tau, radius, background)
        self.out_dir = out_dir
        self.sum = self.count = self.rect = None
        self.frames = 0
        self.device_sum = self.device_count = None     # the loop's device planes, between ``begin`` and ``finish``

    def begin(self, device, rect, shape=(352, 1216)):
        """Zeroed device planes for a new loop on ``device``; ``rect``: the rectangle the loop evaluates."""
        import torch
        self.device_sum = torch.zeros(shape, device=device, dtype=torch.float64)
        self.device_count = torch.zeros(shape, device=device, dtype=torch.int32).view(torch.uint32)
        self.rect, self.frames = tuple(int(v) for v in rect), 0
        self.sum = self.count = None

    def download(self):
        """Queue the copies of the device planes into pinned host buffers on the current stream, without synchronising."""
        import torch
        self._host = (torch.empty(self.device_sum.shape, dtype=torch.float64, pin_memory=True),
                      torch.empty(self.device_count.shape, dtype=torch.int32, pin_memory=True))
        self._host[0].copy_(self.device_sum, non_blocking=True)
        self._host[1].copy_(self.device_count.view(torch.int32), non_blocking=True)

    def finish(self):
        """After the stream of ``download`` has been synchronised: the planes as numpy arrays -> ``self``."""
        self.sum = self._host[0].numpy().copy()
        self.count = self._host[1].numpy().view(np.uint32).copy()
        self.device_sum = self.device_count = self._host = None
        return self

    def add(self, other_sum, other_count, frames=0):
        """Another shard's planes onto these (``multi_gpu_test`` adds the ranks' in rank order: ``count`` adds exactly)."""
        self.sum = self.sum + np.asarray(other_sum, np.float64)
        self.count = self.count + np.asarray(other_count, np.uint32)
        self.frames += int(frames)

    def _planes(self):
        if self.sum is None:
            raise RuntimeError('ErrorMaps holds no planes yet: run single_gpu_test(..., device_eval=True, errors=this) first')
        return self.sum, self.count

    def mean(self):
        """(352, 1216) float64: the mean abs-rel error of the returns at each pixel, NaN where no return was counted."""
        s, n = self._planes()
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(n > 0, s / n, np.nan)

    def rows(self, step=1):
        """``(mean, count)`` per band of ``step`` image rows: the mean abs-rel error of all returns in the rows (NaN where none) and their
        number, arrays of ``ceil(352 / step)`` entries."""
        s, n = self._planes()
        step = int(step)
        if step < 1:
            raise ValueError(f'rows: step must be a positive number of image rows, got {step}')
        starts = range(0, s.shape[0], step)
        tot = np.array([s[r:r + step].sum() for r in starts], np.float64)
        cnt = np.array([n[r:r + step].sum(dtype=np.int64) for r in starts], np.int64)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(cnt > 0, tot / cnt, np.nan), cnt

    def save(self, out_dir):
        """``out_dir/summary.npz`` (``sum``, ``count``, ``tau``, ``rect``, ``frames``) and ``out_dir/mean_abs_rel.png``: the band of
        ``mean() / tau`` in the error images' colours, black where no return was counted."""
        import os
        from PIL import Image
        from ..utils.error_bands import ERROR_COLOURS, error_bands
        s, n = self._planes()
        os.makedirs(out_dir, exist_ok=True)
        np.savez(os.path.join(out_dir, 'summary.npz'), sum=s, count=n, tau=np.float64(self.tau), rect=np.array(self.rect, np.int64),
                 frames=np.int64(self.frames))
        mean = self.mean()
        picture = np.zeros(s.shape + (3,), np.uint8)
        hit = n > 0
        picture[hit] = ERROR_COLOURS[error_bands((mean[hit] / self.tau).astype(np.float32))]
        Image.fromarray(picture).save(os.path.join(out_dir, 'mean_abs_rel.png'), compress_level=1)      # ERROR_COLOURS is RGB

    def __repr__(self):
        return f'ErrorMaps(out_dir={self.out_dir!r}, tau={self.tau}, radius={self.radius}, background={self.background})'


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
