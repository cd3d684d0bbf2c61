"""KITTI Eigen-split dataset for monocular depth with the ground-embedding channels.

Restates depth/datasets/kitti.py:102-620 for the path the GEDepth configs use: split-file parsing (pairs with depth
``None`` are dropped, entries sorted by file name), the per-date calibration tables handed to the pipeline, train / test
sample preparation, and the evaluation protocol (KB crop of the ground truth, Garg / Eigen crop mask, per-image metrics,
nan-mean summary).  The reference's experimental ``mask_pe`` / ``mask_pe_gt`` evaluation variants are not carried.
"""
import os.path as osp
import warnings
from collections import OrderedDict

import numpy as np
from PIL import Image
from torch.utils.data import Dataset

from ..core.evaluation import METRIC_NAMES, metrics, pre_eval_to_metrics
from ..utils.pinned import PinnedUpload
from .builder import DATASETS
from .pipelines import Compose

# P_rect_02 of the five recording days (kitti.py:171-195 / :260-293); 3x4, the 3x3 left block is K
_P_RECT = {
    '2011_09_26': [[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01],
                   [0.0, 0.0, 1.0, 2.745884e-03]],
    '2011_09_28': [[7.070493e+02, 0.0, 6.040814e+02, 4.575831e+01], [0.0, 7.070493e+02, 1.805066e+02, -3.454157e-01],
                   [0.0, 0.0, 1.0, 4.981016e-03]],
    '2011_09_29': [[7.183351e+02, 0.0, 6.003891e+02, 4.450382e+01], [0.0, 7.183351e+02, 1.815122e+02, -5.951107e-01],
                   [0.0, 0.0, 1.0, 2.616315e-03]],
    '2011_09_30': [[7.070912e+02, 0.0, 6.018873e+02, 4.688783e+01], [0.0, 7.070912e+02, 1.831104e+02, 1.178601e-01],
                   [0.0, 0.0, 1.0, 6.203223e-03]],
    '2011_10_03': [[7.188560e+02, 0.0, 6.071928e+02, 4.538225e+01], [0.0, 7.188560e+02, 1.852157e+02, -1.130887e-01],
                   [0.0, 0.0, 1.0, 3.779761e-03]],
}


def _one(t):
    """A one-frame argument as the batch of one ``KITTIDataset._reduce_device`` takes (a view); None stays None."""
    return None if t is None else t[None]


@DATASETS.register_module()
class KITTIDataset(Dataset):
    """Layout (reference docstring, kitti.py:103-134): ``data_root/input/<date>/<drive>/image_02/data/*.png``,
    ``data_root/gt_depth/<drive>/proj_depth/groundtruth/image_02/*.png`` (uint16, metres * 256), split lines
    ``<image> <depth|None> <focal>``; plus ``input/<date>/pe/pe_165.npy`` and ``slope_range_5_5_interval_1/...npz``."""
    device_protocol = 'kitti'                    # the front end of apis/inference.py that ``device_eval`` runs this split through

    def __init__(self, pipeline, img_dir, ann_dir=None, split=None, data_root=None, test_mode=False, depth_scale=256,
                 garg_crop=True, eigen_crop=False, min_depth=1e-3, max_depth=80, mask_pe=False, mask_pe_gt=False):
        if mask_pe or mask_pe_gt:
            raise NotImplementedError('mask_pe / mask_pe_gt evaluation variants are outside the GEDepth hot path')
        self.pipeline = Compose(pipeline)
        self.img_dir, self.ann_dir, self.split, self.data_root = img_dir, ann_dir, split, data_root
        self.test_mode, self.depth_scale = test_mode, depth_scale
        self.garg_crop, self.eigen_crop, self.min_depth, self.max_depth = garg_crop, eigen_crop, min_depth, max_depth
        if self.data_root is not None:
            if not (self.img_dir is None or osp.isabs(self.img_dir)):
                self.img_dir = osp.join(self.data_root, self.img_dir)
            if not (self.ann_dir is None or osp.isabs(self.ann_dir)):
                self.ann_dir = osp.join(self.data_root, self.ann_dir)
        self.img_infos = self.load_annotations(self.img_dir, self.ann_dir, self.split)

    def __len__(self):
        return len(self.img_infos)

    def load_annotations(self, img_dir, ann_dir, split):
        if split is None:
            raise NotImplementedError('Split should be specified')
        self.invalid_depth_num = 0
        infos = []
        with open(split) as f:
            for line in f:
                parts = line.strip().split(' ')
                if not parts or not parts[0]:
                    continue
                info = dict()
                if ann_dir is not None:
                    if parts[1] == 'None':
                        self.invalid_depth_num += 1
                        continue
                    info['ann'] = dict(depth_map=parts[1])
                info['filename'] = parts[0]
                infos.append(info)
        return sorted(infos, key=lambda x: x['filename'])

    def get_ann_info(self, idx):
        return self.img_infos[idx]['ann']

    def pre_pipeline(self, results):
        results['depth_fields'] = []
        results['img_prefix'] = self.img_dir
        results['depth_prefix'] = self.ann_dir
        results['depth_scale'] = self.depth_scale
        results['cam_intrinsic_dict_for_nromal'] = {d: np.array(p)[:, :3] for d, p in _P_RECT.items()}
        results['cam_intrinsic_dict'] = {d: [list(r) for r in p] for d, p in _P_RECT.items()}

    def __getitem__(self, idx):
        results = dict(img_info=self.img_infos[idx], ann_info=self.get_ann_info(idx))
        self.pre_pipeline(results)
        return self.pipeline(results)

    prepare_train_img = prepare_test_img = __getitem__

    def engine_frame(self, index):
        """Split entry ``index`` as the keyword arguments of ``DepthInferencer.__call__``."""
        return dict(img=osp.join(self.img_dir, self.img_infos[index]['filename']))

    def format_results(self, results, imgfile_prefix=None, indices=None, **kwargs):
        results[0] = (results[0] * self.depth_scale).astype(np.uint16)
        return results

    def _gt(self, index):
        path = osp.join(self.ann_dir, self.img_infos[index]['ann']['depth_map'])
        return np.asarray(Image.open(path), dtype=np.float32) / self.depth_scale

    def get_gt_depth_maps(self):
        for i in range(len(self)):
            yield self._gt(i)

    @staticmethod
    def eval_kb_crop(depth_gt):
        h, w = depth_gt.shape
        top, left = int(h - 352), int((w - 1216) / 2)
        return depth_gt[top:top + 352, left:left + 1216][None]

    def eval_mask(self, depth_gt):
        depth_gt = np.squeeze(depth_gt)
        valid = np.logical_and(depth_gt > self.min_depth, depth_gt < self.max_depth)
        if self.garg_crop or self.eigen_crop:
            gh, gw = depth_gt.shape
            crop = np.zeros(valid.shape)
            if self.garg_crop:
                crop[int(0.40810811 * gh):int(0.99189189 * gh), int(0.03594771 * gw):int(0.96405229 * gw)] = 1
            else:
                crop[int(0.3324324 * gh):int(0.91351351 * gh), int(0.0359477 * gw):int(0.96405229 * gw)] = 1
            valid = np.logical_and(valid, crop)
        return valid[None]

    def eval_rect(self, gh, gw):
        """``(r0, r1, c0, c1)``: the rows / columns of a ``(gh, gw)`` crop that ``eval_mask`` keeps (its own ``int(...)`` expressions); the
        whole crop when neither the Garg nor the Eigen crop is on."""
        if self.garg_crop:
            return int(0.40810811 * gh), int(0.99189189 * gh), int(0.03594771 * gw), int(0.96405229 * gw)
        if self.eigen_crop:
            return int(0.3324324 * gh), int(0.91351351 * gh), int(0.0359477 * gw), int(0.96405229 * gw)
        return 0, gh, 0, gw

    def gt_raw(self, index):
        """Split entry ``index``'s ground-truth PNG as it is on disk, an (H, W) uint16 array at least as large as the KB crop: host work
        only, so a thread may decode it ahead of the device."""
        path = osp.join(self.ann_dir, self.img_infos[index]['ann']['depth_map'])
        raw = np.asarray(Image.open(path))
        if raw.dtype != np.uint16 or raw.ndim != 2:
            raise TypeError(f'{path}: the ground truth must be a 16-bit single-channel PNG, got {raw.dtype} {raw.shape}')
        h, w = raw.shape
        if h < 352 or w < 1216:
            raise ValueError(f'{path}: ground truth {(h, w)} is smaller than the KB crop (352, 1216)')
        return raw

    def _reduce_device(self, what, preds, indices, raws=None, *, sums_rows=None, strata=None, rows=None, grounds=None, errors=None,
                       frames=None, outs=None, count=None):
        """What the six ``pre_eval_device*`` methods do, for n = ``len(indices)`` in 1 .. 8 images, in the words of the public method
        ``what``: ``preds`` a CUDA ``(F >= n, 1, 352, 1216)`` float32 tensor whose first n maps belong to ``indices``.  The n ground-truth
        PNGs go up undivided, as uint16, each through its own reused pinned buffer, on the current stream (``raws``: their ``gt_raw``
        arrays when a thread has decoded them ahead); the KB crop, the Garg / Eigen rectangle and the depth mask are applied by the kernels.
        On these uploads, one call each, in this order:

        * ``sums_rows`` (n rows of a device ``(N, 10)`` float64 buffer): ``ge_depth_metrics_batch`` writes every image's ten metric sums
          (``core.metrics_from_sums`` makes the tuple of ``pre_eval`` from a row);
        * ``strata`` (a ``core.StrataSpec``) with ``rows`` (n (S, 10) blocks of a device (N, S, 10) float64 buffer) and ``grounds`` (the
          frames' raw (H, W) float32 ground depths on the device, what the front end was fed; read only with ``strata.ground``):
          ``ge_depth_metrics_strata_batch`` writes the sums per stratum;
        * ``errors`` (a ``core.ErrorMaps`` after ``begin``): ``ge_error_accumulate_batch`` adds the first ``count`` = m <= n images
          (default: all), in index order, into its planes, and with ``errors.out_dir`` ``ge_error_image_batch`` paints them over
          ``frames`` (the n (uploaded (H, W, 3) uint8 BGR frame, top, left) the engine keeps as ``last_frames``) into the first m blocks of
          ``outs`` (a CUDA (F >= m, 352, 1216, 3) uint8 tensor, made when None) -- returned as (m, 352, 1216, 3), else None.  The loop keeps
          a padded shard's repeated frames out of planes and pictures with ``count``; the metric and strata calls still cover all n.

        Every image's results carry the same bits whatever n it is reduced with.  Does not synchronise: the results are valid once the
        current stream has reached this point."""
        import torch
        from ... import kernels as K
        n, one = len(indices), int(not what.endswith('_batch'))         # the one-frame forms hand in ``pred[None]``
        if not (torch.is_tensor(preds) and preds.is_cuda and preds.dim() == 4 and tuple(preds.shape[1:]) == (1, 352, 1216)
                and preds.shape[0] >= n and preds.dtype == torch.float32):
            takes = 'a CUDA (1, 352, 1216) float32 prediction' if one else f'a CUDA (F >= {n}, 1, 352, 1216) float32 tensor'
            raise TypeError(f'{what} takes {takes}, got {tuple(preds.shape[one:]) if torch.is_tensor(preds) else type(preds)}')
        if not 1 <= n <= 8 or (sums_rows is not None and tuple(sums_rows.shape) != (n, 10)):
            raise ValueError(f'{what} takes 1 .. 8 images and one (10,) row each, got {n} and '
                             f'{None if sums_rows is None else tuple(sums_rows.shape)}')
        if strata is not None:
            if rows is None or tuple(rows.shape) != (n, strata.count, 10):
                raise ValueError(f'{what}: strata need one ({strata.count}, 10) block for each of {n} images, got '
                                 f'{None if rows is None else tuple(rows.shape)}')
            if strata.ground and (grounds is None or len(grounds) != n or any(g is None for g in grounds)):
                raise ValueError(f'{what}: spec.ground needs every frame\'s ground depth')
        if sums_rows is None and strata is None and errors is None:
            raise ValueError(f'{what}: no rows to reduce into')
        m = 0
        if errors is not None:
            m = n if count is None else int(count)
            if not 0 <= m <= n:
                raise ValueError(f'{what}: count must lie in 0 .. {n}, got {count}')
            if errors.device_sum is None:
                raise ValueError(f'{what}: errors holds no device planes (ErrorMaps.begin makes them)')
            if errors.out_dir and m and (frames is None or len(frames) != n):
                raise ValueError(f'{what}: {n} images need their {n} uploaded frames')
        raws = [self.gt_raw(i) for i in indices] if raws is None else raws
        tops = [int(r.shape[0] - 352) for r in raws]                    # eval_kb_crop
        lefts = [int((r.shape[1] - 1216) / 2) for r in raws]
        if m and errors.out_dir:
            for (bgr, ftop, fleft), raw, top, left in zip(frames, raws, tops, lefts):
                if (ftop, fleft) != (top, left) or tuple(bgr.shape[:2]) != tuple(raw.shape):
                    raise ValueError(f'{what}: a frame {tuple(bgr.shape[:2])} at {(ftop, fleft)} is not its ground truth\'s '
                                     f'{tuple(raw.shape)} at {(top, left)}')
        uploads = self.__dict__.setdefault('_gt_uploads', [])          # one staging buffer per slot: n copies are in flight at once
        while len(uploads) < n:
            uploads.append(PinnedUpload())
        devs = [up(raw, preds.device) for up, raw in zip(uploads, raws)]
        rect, limits = self.eval_rect(352, 1216), (self.depth_scale, self.min_depth, self.max_depth)
        if sums_rows is not None:
            K.depth_metric_sums_batch(preds, devs, tops, lefts, rect, *limits, sums_rows)
        if strata is not None:
            K.depth_metric_sums_strata_batch(preds, devs, tops, lefts, rect, *limits, rows, strata.edges,
                                             list(grounds) if strata.ground else None, strata.ground_tol)
        if not m:
            return None
        K.error_accumulate_batch(preds, devs[:m], tops[:m], lefts[:m], rect, *limits, errors.device_sum, errors.device_count)
        errors.frames += m
        if not errors.out_dir:
            return None
        out, _ = K.error_image_batch(preds, devs[:m], [f[0] for f in frames[:m]], tops[:m], lefts[:m], rect, *limits, errors.tau,
                                     errors.radius, errors.background, want_err=False, out=outs)
        return out[:m]

    # The public forms: adapters over ``_reduce_device`` (its docstring is the contract).  Each calls the core and never a sibling, so
    # one replaced on an instance is not entered through another.
    def pre_eval_device_batch(self, preds, indices, sums_rows, raws=None):
        """The metric sums of n = ``len(indices)`` <= 8 images into ``sums_rows`` (n, 10): one ``ge_depth_metrics_batch`` call."""
        self._reduce_device('pre_eval_device_batch', preds, indices, raws, sums_rows=sums_rows)

    def pre_eval_device_strata_batch(self, preds, indices, rows, spec, grounds, raws=None, sums_rows=None):
        """The sums per stratum of ``spec`` into ``rows`` (n, S, 10): one ``ge_depth_metrics_strata_batch`` call; ``sums_rows``: also
        ``pre_eval_device_batch``'s own call, on the same uploads."""
        self._reduce_device('pre_eval_device_strata_batch', preds, indices, raws, sums_rows=sums_rows, strata=spec, rows=rows, grounds=grounds)

    def pre_eval_device_errors_batch(self, preds, indices, errors, frames, outs=None, raws=None, *, sums_rows=None, strata=None, rows=None,
                                     grounds=None, count=None):
        """The first ``count`` (default: all n) images into the planes of ``errors`` and, with ``errors.out_dir``, into their pictures,
        which are returned (else None); ``sums_rows``, ``strata`` / ``rows`` / ``grounds``: also the calls of the two forms above."""
        return self._reduce_device('pre_eval_device_errors_batch', preds, indices, raws, sums_rows=sums_rows, strata=strata, rows=rows,
                                   grounds=grounds, errors=errors, frames=frames, outs=outs, count=count)

    def pre_eval_device(self, pred, index, sums_row):
        """``pre_eval_device_batch`` of one image: ``pred`` a CUDA (1, 352, 1216) float32 map, ``sums_row`` one (10,) row."""
        self._reduce_device('pre_eval_device', _one(pred), [index], sums_rows=_one(sums_row))

    def pre_eval_device_strata(self, pred, index, rows, spec, ground, sums_row=None):
        """``pre_eval_device_strata_batch`` of one image: ``rows`` one (S, 10) block, ``ground`` the frame's ground depth."""
        self._reduce_device('pre_eval_device_strata', _one(pred), [index], sums_rows=_one(sums_row), strata=spec, rows=_one(rows),
                            grounds=[ground])

    def pre_eval_device_errors(self, pred, index, errors, frame, out=None, raw=None, *, sums_row=None, strata=None, rows=None, ground=None):
        """``pre_eval_device_errors_batch`` of one image: ``frame`` what the engine keeps as ``last_frame``, ``out`` a CUDA
        (352, 1216, 3) uint8 tensor (made when None); returns the (352, 1216, 3) picture, or None without ``errors.out_dir``."""
        got = self._reduce_device('pre_eval_device_errors', _one(pred), [index], None if raw is None else [raw], sums_rows=_one(sums_row),
                                  strata=strata, rows=_one(rows), grounds=[ground], errors=errors, frames=[frame], outs=_one(out))
        return None if got is None else got[0]

    def pre_eval_device_sweep(self, preds, index, out_rows, raw=None):
        """The prior sweep's reduction: the V = ``out_rows.shape[0]`` <= 8 first maps of ``preds`` (a CUDA (F >= V, 1, 352, 1216) float32
        tensor: ONE frame under V ground priors, ``BatchDepthInferencer.sweep``) against split entry ``index``'s ground truth ->
        ``out_rows`` (V, 10), row v the ten metric sums of map v.  The ground-truth PNG goes up ONCE (``raw``: its ``gt_raw`` array when a
        thread has decoded it ahead) and ONE ``ge_depth_metrics_batch`` call reads it through V table rows that all point at that upload,
        so row v carries the bits ``pre_eval_device`` gives map v.  On the current stream, without synchronising."""
        import torch
        from ... import kernels as K
        what = 'pre_eval_device_sweep'
        if not (torch.is_tensor(out_rows) and out_rows.dim() == 2 and out_rows.shape[1] == 10 and 1 <= out_rows.shape[0] <= 8):
            raise ValueError(f'{what} takes 1 .. 8 variants and one (10,) row each, got '
                             f'{tuple(out_rows.shape) if torch.is_tensor(out_rows) else type(out_rows)}')
        V = out_rows.shape[0]
        if not (torch.is_tensor(preds) and preds.is_cuda and preds.dim() == 4 and tuple(preds.shape[1:]) == (1, 352, 1216)
                and preds.shape[0] >= V and preds.dtype == torch.float32):
            raise TypeError(f'{what} takes a CUDA (F >= {V}, 1, 352, 1216) float32 tensor, got '
                            f'{tuple(preds.shape) if torch.is_tensor(preds) else type(preds)}')
        raw = self.gt_raw(index) if raw is None else raw
        top, left = int(raw.shape[0] - 352), int((raw.shape[1] - 1216) / 2)        # eval_kb_crop
        uploads = self.__dict__.setdefault('_gt_uploads', [])
        if not uploads:
            uploads.append(PinnedUpload())
        dev = uploads[0](raw, preds.device)
        K.depth_metric_sums_batch(preds, [dev] * V, [top] * V, [left] * V, self.eval_rect(352, 1216), self.depth_scale, self.min_depth,
                                  self.max_depth, out_rows)

    def evaluate_sweep(self, rows, spec, logger=None):
        """``rows`` (N, V, 10) float64 from the sweep loop, ``spec`` its ``core.PriorSweep`` -> ``{variant name: {metric: value}}``: the
        nine metrics as the nan-mean over images of ``metrics_from_sums(row)`` — the convention of ``evaluate``'s headline numbers, so the
        baseline line is what ``evaluate`` prints for the loop's ``results`` — and, for every variant but the baseline, ``d_abs_rel``,
        ``d_rmse`` and ``d_a1``: its value minus the baseline's.  Prints one line per variant."""
        from ..core.evaluation import metrics_from_sums
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[1:] != (spec.count, 10):
            raise ValueError(f'evaluate_sweep takes (N, {spec.count}, 10) rows for {spec!r}, got {rows.shape}')
        table = OrderedDict()
        for v, name in enumerate(spec.names):
            tuples = [metrics_from_sums(r) for r in rows[:, v]]
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)                     # a split without a counted pixel: NaN, as ``evaluate``
                table[name] = OrderedDict((k, float(np.nanmean([t[i] for t in tuples])) if tuples else float('nan'))
                                          for i, k in enumerate(METRIC_NAMES))
        base = table[spec.names[0]]
        for name in spec.names[1:]:
            for k in ('abs_rel', 'rmse', 'a1'):
                table[name][f'd_{k}'] = table[name][k] - base[k]
        width = max(len(name) for name in table)
        deltas = ('d_abs_rel', 'd_rmse', 'd_a1')
        lines = ['Prior sweep:', ' | '.join([' ' * width] + [f'{k:>8s}' for k in METRIC_NAMES] + [f'{k:>9s}' for k in deltas])]
        for name, entry in table.items():
            lines.append(' | '.join([f'{name:<{width}s}'] + [f'{entry[k]:8.4f}' for k in METRIC_NAMES]
                                    + [f'{entry[k]:+9.4f}' if k in entry else ' ' * 9 for k in deltas]))
        (logger.info if logger is not None and hasattr(logger, 'info') else print)('\n'.join(lines))
        return table

    def evaluate_strata(self, rows, spec, logger=None):
        """``rows`` (N, S, 10) float64 from the device loop -> ``{'<stratum>.<metric>': value}`` (the nine metrics, ``pixels`` and ``images``
        of ``core.strata_table``); prints the table."""
        from ..core.evaluation import strata_table
        table = strata_table(rows, spec, self.min_depth, self.max_depth)
        cols = METRIC_NAMES + ('pixels', 'images')
        width = max(len(name) for name in table)
        lines = ['Strata:', ' | '.join([' ' * width] + [f'{k:>8s}' for k in cols])]
        for name, entry in table.items():
            lines.append(' | '.join([f'{name:<{width}s}'] + [f'{entry[k]:8.4f}' for k in METRIC_NAMES]
                                    + [f'{entry["pixels"]:8.4f}', f'{entry["images"]:8d}']))
        (logger.info if logger is not None and hasattr(logger, 'info') else print)('\n'.join(lines))
        return {f'{name}.{k}': v for name, entry in table.items() for k, v in entry.items()}

    def pre_eval(self, preds, indices):
        """Per-image metric tuples for predictions ``(1, 352, 1216)`` (kitti.py:502-552)."""
        if not isinstance(indices, list):
            indices = [indices]
        if not isinstance(preds, list):
            preds = [preds]
        out_metrics, out_preds = [], []
        for pred, index in zip(preds, indices):
            gt = self.eval_kb_crop(self._gt(index))
            mask = self.eval_mask(gt)
            out_metrics.append(metrics(gt[mask], pred[mask], min_depth=self.min_depth, max_depth=self.max_depth))
            out_preds.append(pred)
        return out_metrics, out_preds

    def evaluate(self, results, metric='eigen', logger=None, **kwargs):
        """results: per-image metric tuples from ``pre_eval`` or a list of predicted depth maps."""
        if len(results) and isinstance(results[0], np.ndarray):
            pre = []
            for gt, pred in zip(self.get_gt_depth_maps(), results):
                gt = self.eval_kb_crop(gt)
                mask = self.eval_mask(gt)
                pre.append(metrics(gt[mask], pred[mask], min_depth=self.min_depth, max_depth=self.max_depth))
            results = pre
        ret = pre_eval_to_metrics(results)
        summary = OrderedDict((k, np.round(np.nanmean(v), 4)) for k, v in ret.items())
        text = 'Summary:\n' + ' | '.join(f'{k:>8s}' for k in METRIC_NAMES) + '\n' + ' | '.join(f'{summary[k]:8.4f}' for k in METRIC_NAMES)
        (logger.info if logger is not None and hasattr(logger, 'info') else print)(text)
        return dict(ret)
