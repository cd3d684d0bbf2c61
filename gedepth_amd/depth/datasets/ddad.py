"""DDAD (front + side cameras) dataset with the ground-embedding channels — restates depth/datasets/ddad.py:31-310:
split lines ``<image> <depth .npz>`` filtered by camera, per-camera intrinsics, and the evaluation protocol (prediction
resized bilinearly, align_corners=True, to the full-resolution ground truth; valid where min_depth < gt < max_depth)."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from ..core.evaluation import METRIC_NAMES, metrics, pre_eval_to_metrics
from ..utils.pinned import PinnedUpload
from .builder import DATASETS
from .pipelines import Compose
from .pipelines.loading import ddad_camera_of

_CAM_K = {
    'CAMERA_01': [[2.1815303e+03, 0.0, 9.2802191e+02, 0], [0.0, 2.1816035e+03, 6.1595679e+02, 0], [0.0, 0.0, 1.0, 0]],
    'CAMERA_05': [[1.0570685e+03, 0.0, 9.6468347e+02, 0], [0.0, 1.0559746e+03, 5.8866125e+02, 0], [0.0, 0.0, 1.0, 0]],
    'CAMERA_06': [[1.0607557e+03, 0.0, 9.4655847e+02, 0], [0.0, 1.0592549e+03, 6.1140710e+02, 0], [0.0, 0.0, 1.0, 0]],
    'CAMERA_09': [[1.0634580e+03, 0.0, 9.4466577e+02, 0], [0.0, 1.0652224e+03, 6.1269843e+02, 0], [0.0, 0.0, 1.0, 0]],
}


@DATASETS.register_module()
class DDADDataset(Dataset):
    device_protocol = 'ddad'                     # the front end of apis/inference.py that ``device_eval`` runs this split through

    def __init__(self, pipeline, cameras=('CAMERA_01', 'CAMERA_05', 'CAMERA_06', 'CAMERA_07', 'CAMERA_08', 'CAMERA_09'),
                 split=None, test_mode=False, garg_crop=False, eigen_crop=False, min_depth=1e-3, max_depth=200):
        self.garg_crop, self.eigen_crop, self.cameras = garg_crop, eigen_crop, list(cameras)
        self.pipeline = Compose(pipeline)
        self.split, self.test_mode, self.min_depth, self.max_depth = split, test_mode, min_depth, max_depth
        self.img_infos = self.load_annotations(split)

    def __len__(self):
        return len(self.img_infos)

    def load_annotations(self, split):
        if split is None:
            raise NotImplementedError('Split should be specified')
        infos = []
        with open(split) as f:
            for line in f:
                parts = line.strip().split(' ')
                if len(parts) < 2:
                    continue
                if ddad_camera_of(parts[1]) in self.cameras:
                    infos.append(dict(filename=parts[0], ann=dict(depth_map=parts[1].replace('depth_val', 'depth'))))
        return sorted(infos, key=lambda x: x['filename'])

    def get_ann_info(self, idx):
        return self.img_infos[idx]['ann']

    def pre_pipeline(self, results):
        results['depth_fields'] = []
        results['cam_intrinsic_dict'] = {c: [list(r) for r in k] for c, k in _CAM_K.items()}

    def __getitem__(self, idx):
        results = dict(img_info=self.img_infos[idx], ann_info=self.get_ann_info(idx))
        self.pre_pipeline(results)
        return self.pipeline(results)

    prepare_train_img = prepare_test_img = __getitem__

    def camera_of(self, index):
        return ddad_camera_of(self.img_infos[index]['ann']['depth_map'])

    def engine_frame(self, index):
        """Split entry ``index`` as the keyword arguments of ``DepthInferencer.__call__``: the split holds full paths."""
        return dict(img=self.img_infos[index]['filename'], camera=self.camera_of(index))

    def format_results(self, results, imgfile_prefix=None, indices=None, **kwargs):
        results[0] = results[0].astype(np.uint16)
        return results

    def get_gt_depth_maps(self):
        for info in self.img_infos:
            yield np.load(info['ann']['depth_map'])['depth']

    def eval_mask(self, depth_gt):
        depth_gt = np.squeeze(depth_gt)
        return np.logical_and(depth_gt > self.min_depth, depth_gt < self.max_depth)[None]

    def pre_eval(self, preds, indices):
        if not isinstance(indices, list):
            indices = [indices]
        if not isinstance(preds, list):
            preds = [preds]
        out_metrics, out_preds = [], []
        for pred, index in zip(preds, indices):
            gt = np.load(self.img_infos[index]['ann']['depth_map'])['depth'].astype(np.float32)
            pred = F.interpolate(torch.from_numpy(np.asarray(pred, dtype=np.float32))[None], size=gt.shape, mode='bilinear',
                                 align_corners=True)[0].numpy()
            gt = gt[None]
            mask = self.eval_mask(gt)
            out_metrics.append(metrics(gt[mask], pred[mask], min_depth=self.min_depth, max_depth=self.max_depth))
            out_preds.append(pred)
        return out_metrics, out_preds

    def pre_eval_device(self, pred, index, sums_row):
        """``pre_eval_device_batch`` of one image: ``pred`` a CUDA ``(1, Hd, Wd)`` float32 map, ``sums_row`` one (10,) row of the device
        ``(N, 10)`` float64 buffer."""
        if not (torch.is_tensor(pred) and pred.is_cuda and pred.dim() == 3 and pred.shape[0] == 1 and pred.dtype == torch.float32):
            raise TypeError('pre_eval_device takes a CUDA (1, Hd, Wd) float32 prediction, got '
                            f'{(tuple(pred.shape), pred.dtype, pred.device.type) if torch.is_tensor(pred) else type(pred)}')
        self._reduce_device(pred[None], [index], sums_row[None], [self.gt_raw(index)])

    def gt_raw(self, index):
        """Split entry ``index``'s ground truth as the device evaluation uploads it, the ``.npz``'s ``depth`` as an (H, W) float32 array
        (float32 as in ``pre_eval``): host work only (inflating the file releases the GIL), so a thread may load it ahead of the device."""
        path = self.img_infos[index]['ann']['depth_map']
        gt = np.load(path)['depth']
        if gt.ndim != 2:
            raise TypeError(f'{path}: the ground truth must be a 2-D depth array, got shape {gt.shape}')
        return np.ascontiguousarray(gt, dtype=np.float32)

    def pre_eval_device_batch(self, preds, indices, sums_rows, raws=None):
        """``pre_eval`` of n = ``len(indices)`` <= 8 images where the predictions already are: ``preds`` a CUDA ``(F, 1, Hd, Wd)`` float32
        tensor whose first n maps belong to ``indices``, ``sums_rows`` n rows of a device ``(N, 10)`` float64 buffer that receive the
        images' metric sums (``core.metrics_from_sums`` makes the tuple of ``pre_eval`` from a row); a row carries the same bits whatever
        n its image is reduced with.  The n ground truths go up as float32, each through its own reused pinned buffer, on the current
        stream (``raws``: their ``gt_raw`` arrays when a thread has loaded them ahead); then one ``ge_depth_metrics_resized_batch`` call
        (two launches) per run of consecutive images whose ground truths have one size -- a DDAD split has one, so one call.  The kernel
        resamples the prediction at the ground-truth pixels that count (bilinear, align_corners=True, in float32: not bit-equal to
        ``F.interpolate`` on the CPU, see include/gedepth_ddad.h) and reduces in the same pass, so the resized map is never written.
        Does not synchronise: the rows are valid once the current stream has reached this point."""
        n = len(indices)
        if not (torch.is_tensor(preds) and preds.is_cuda and preds.dim() == 4 and preds.shape[1] == 1 and preds.shape[0] >= n
                and preds.dtype == torch.float32):
            raise TypeError(f'pre_eval_device_batch takes a CUDA (F >= {n}, 1, Hd, Wd) float32 tensor, got '
                            f'{(tuple(preds.shape), preds.dtype, preds.device.type) if torch.is_tensor(preds) else type(preds)}')
        if not 1 <= n <= 8 or tuple(sums_rows.shape) != (n, 10):
            raise ValueError(f'pre_eval_device_batch takes 1 .. 8 images and one (10,) row each, got {n} and {tuple(sums_rows.shape)}')
        raws = [self.gt_raw(i) for i in indices] if raws is None else raws
        if len(raws) != n:
            raise ValueError(f'{len(raws)} ground truths for {n} images')
        self._reduce_device(preds, indices, sums_rows, raws)

    def _reduce_device(self, preds, indices, sums_rows, raws):
        """The uploads and kernel calls of ``pre_eval_device_batch``, behind its checks."""
        from ... import kernels as K
        n = len(indices)
        uploads = self.__dict__.setdefault('_gt_uploads', [])          # one staging buffer per slot, made on first use: n copies are in flight at once
        while len(uploads) < n:
            uploads.append(PinnedUpload())
        devs = [up(raw, preds.device) for up, raw in zip(uploads, raws)]
        start = 0
        while start < n:                                               # runs of equal ground-truth size
            end = start + 1
            while end < n and raws[end].shape == raws[start].shape:
                end += 1
            K.depth_metric_sums_resized_batch(preds[start:end], devs[start:end], self.min_depth, self.max_depth, sums_rows[start:end])
            start = end

    def evaluate(self, results, metric='eigen', logger=None, **kwargs):
        if len(results) and isinstance(results[0], np.ndarray):
            results = self.pre_eval(list(results), list(range(len(results))))[0]
        ret = pre_eval_to_metrics(results)
        summary = OrderedDict((k, np.round(np.nanmean(v), 4)) for k, v in ret.items())
        text = 'Summary:\n' + ' | '.join(f'{k:>8s}' for k in METRIC_NAMES) + '\n' + ' | '.join(f'{summary[k]:8.4f}' for k in METRIC_NAMES)
        (logger.info if logger is not None and hasattr(logger, 'info') else print)(text)
        return dict(ret)
