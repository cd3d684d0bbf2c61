"""BaseDepther: call protocol, train_step and loss parsing (mirror of depth/models/depther/base.py:16-204).

MI355X-first difference: the reference does one ``all_reduce`` + ``.item()`` per logged scalar per
iteration (base.py:197-202 — 2-3 host syncs per step).  Here the scalars are stacked into one tensor, reduced
with ONE collective, and only brought to the host when a logger actually reads them (``DeferredLogVars``).
"""
import os
import os.path as osp
import warnings
from abc import ABCMeta, abstractmethod
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

from ....mmrt.bricks import BaseModule


class DeferredLogVars(OrderedDict):
    """name -> float mapping whose values live in one device tensor until first read."""

    def __init__(self, names, values):
        super().__init__((n, None) for n in names)
        self._names, self._tensor = list(names), values

    def _materialize(self):
        if self._tensor is not None:
            vals = self._tensor.detach().float().cpu().tolist()     # the single host sync
            self._tensor = None
            for n, v in zip(self._names, vals):
                super().__setitem__(n, v)

    def __getitem__(self, k):
        self._materialize()
        return super().__getitem__(k)

    def get(self, k, default=None):
        self._materialize()
        return super().get(k, default)

    def items(self):
        self._materialize()
        return super().items()

    def values(self):
        self._materialize()
        return super().values()

    def tensor(self):
        """Device tensor of the (already all-reduced) values, or None once materialised."""
        return self._tensor


_PIL_SAVE_ARGS = {'png': dict(compress_level=1), 'jpg': dict(quality=95), 'jpeg': dict(quality=95)}     # OpenCV's imwrite defaults
_warned_no_display = False


def _to_host(depth):
    return depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)


def _imwrite_bgr(bgr, out_file):
    """``mmcv.imwrite(bgr, out_file)``: the BGR array is stored as an RGB image (format from the extension), parent directories created."""
    from PIL import Image
    d = osp.dirname(osp.abspath(out_file))
    os.makedirs(d, exist_ok=True)
    ext = osp.splitext(out_file)[1][1:].lower()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(out_file, **_PIL_SAVE_ARGS.get(ext, {}))


class BaseDepther(BaseModule, metaclass=ABCMeta):

    def __init__(self, init_cfg=None):
        super().__init__(init_cfg)
        self.fp16_enabled = False

    @property
    def with_neck(self):
        return hasattr(self, 'neck') and self.neck is not None

    @property
    def with_auxiliary_head(self):
        return hasattr(self, 'auxiliary_head') and self.auxiliary_head is not None

    @property
    def with_decode_head(self):
        return hasattr(self, 'decode_head') and self.decode_head is not None

    @abstractmethod
    def extract_feat(self, imgs):
        pass

    @abstractmethod
    def encode_decode(self, img, img_metas):
        pass

    @abstractmethod
    def forward_train(self, imgs, img_metas, **kwargs):
        pass

    @abstractmethod
    def simple_test(self, img, img_meta, **kwargs):
        pass

    @abstractmethod
    def aug_test(self, imgs, img_metas, **kwargs):
        pass

    def forward_test(self, imgs, img_metas, **kwargs):
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError(f'{name} must be a list, but got {type(var)}')
        num_augs = len(imgs)
        if num_augs != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        for img_meta in img_metas:
            for key in ('ori_shape', 'img_shape', 'pad_shape'):
                vals = [m[key] for m in img_meta if key in m]
                assert all(v == vals[0] for v in vals)
        if num_augs == 1:
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def train_step(self, data_batch, optimizer=None, **kwargs):
        losses = self(**data_batch)
        real_losses = {k: v for k, v in losses.items() if 'img' not in k}
        log_imgs = {k: v for k, v in losses.items() if 'img' in k}
        loss, log_vars = self._parse_losses(real_losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data_batch['img_metas']), log_imgs=log_imgs)

    def val_step(self, data_batch, **kwargs):
        return self(**data_batch, **kwargs)

    def show_result(self, img, result, win_name='', show=False, wait_time=0, out_file=None, format_only=False):
        """Write ``depth = result[0]`` (base.py:206-247 of the reference, its behaviour rather than its docstring).

        ``format_only``: ``np.save(out_file, depth)``, the raw map.  Otherwise ``out_file`` gets ``colorize(depth)`` over
        ``[decode_head.min_depth, decode_head.max_depth]`` as an image whose pixels are matplotlib's RGB (PNG written like OpenCV's
        default).  Parent directories of ``out_file`` are created.  ``show``: there is no display here, so it only warns (once); ``img``
        (a path or an array) only fed that display and is not read.  With neither ``show`` nor ``out_file`` it warns and returns
        ``depth`` unchanged."""
        global _warned_no_display
        depth = result[0]
        if show and not _warned_no_display:
            warnings.warn('show_result(show=True): no display support in gedepth_amd; nothing is shown (use out_file)')
            _warned_no_display = True
        if out_file is not None:
            if format_only:
                os.makedirs(osp.dirname(osp.abspath(out_file)), exist_ok=True)
                np.save(out_file, _to_host(depth))
            else:
                from ...utils import colorize
                bgr = _to_host(colorize(depth, vmin=self.decode_head.min_depth, vmax=self.decode_head.max_depth)).squeeze()
                if bgr.ndim != 3:
                    raise ValueError(f'show_result writes one image: result[0] must be one depth map, got shape {np.shape(depth)}')
                _imwrite_bgr(bgr, out_file)
        if not (show or out_file):
            warnings.warn('show==False and out_file is not specified, only result depth will be returned')
            return depth

    def show_ground(self, result, out_file, format_only=False):
        """Write one frame's ground maps, ``result`` = a dict of ``inference_ground`` / ``DepthInferencer.ground_maps`` (host arrays or
        device tensors).  With ``<stem>`` = ``out_file`` without its extension: ``<stem>_attention.png`` (the ground attention over
        [0, 1]), ``<stem>_slope.png`` (``slope_deg`` over [-5, 5]; skipped when the key is absent: a vanilla model) and
        ``<stem>_ground.png`` (``ground_depth`` over ``[decode_head.min_depth, decode_head.max_depth]``), each ``colorize``d with
        'magma_r' and written as ``show_result`` writes its picture.  ``format_only``: one ``<stem>.npz`` with every array of ``result``
        as it is.  Parent directories are created."""
        stem = osp.splitext(out_file)[0]
        if format_only:
            os.makedirs(osp.dirname(osp.abspath(stem)), exist_ok=True)
            np.savez(stem + '.npz', **{k: _to_host(v) for k, v in result.items()})
            return
        from ...utils import colorize
        head = self.decode_head
        for key, suffix, vmin, vmax in (('attention', 'attention', 0.0, 1.0), ('slope_deg', 'slope', -5.0, 5.0),
                                        ('ground_depth', 'ground', head.min_depth, head.max_depth)):
            if key == 'slope_deg' and key not in result:
                continue
            bgr = _to_host(colorize(result[key], vmin=vmin, vmax=vmax))
            if bgr.ndim != 3:
                raise ValueError(f'show_ground writes one image per map: result[{key!r}] must be (H, W), got shape {np.shape(result[key])}')
            _imwrite_bgr(bgr, f'{stem}_{suffix}.png')

    def save_point_cloud(self,img, result, cam_intrinsic, out_file, top=0, left=0, **cloud_kw):
        """Write ``depth = result[0]`` (a host or device map) as a coloured point cloud, a binary PLY file (``depth.utils.write_ply``): the
        host-map route to ``depth.utils.depth_to_points``, like ``show_result`` for pictures.  ``img``: the frame, a path or an (Hs, Ws, 3)
        uint8 BGR array, whose pixel (top + r, left + c) colours map pixel (r, c) (KB crop: ``top = Hs - 352``, ``left = (Ws - 1216) // 2``).
        ``cam_intrinsic``: 3x3 or 3x4, in FRAME coordinates (the ``cam_intrinsic`` meta of the test pipeline); the crop is subtracted here.
        ``cloud_kw``: ``min_depth`` / ``max_depth`` (default: the decode head's), ``row0``, ``step``, ``alpha``.  Returns the points."""
        from ...apis.inference import _decode
        from ...utils.point_cloud import _fxfycxcy, depth_to_points, records_to_points, write_ply
        depth = result[0]
        if np.ndim(depth) == 3 and np.shape(depth)[0] != 1 or np.ndim(depth) not in (2, 3):
            raise ValueError(f'save_point_cloud writes one cloud: result[0] must be one depth map, got shape {np.shape(depth)}')
        fx, fy, cx, cy = _fxfycxcy(cam_intrinsic)
        K = [[fx, 0.0, cx - left], [0.0, fy, cy - top], [0.0, 0.0, 1.0]]
        cloud_kw.setdefault('min_depth', self.decode_head.min_depth)
        cloud_kw.setdefault('max_depth', self.decode_head.max_depth)
        points = depth_to_points(depth, K, _decode(img), top, left, **cloud_kw)
        if isinstance(points, tuple):
            points = records_to_points(*points)
        write_ply(out_file, points)
        return points

    @staticmethod
    def _parse_losses(losses):
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean()
            elif isinstance(value, list):
                log_vars[name] = sum(v.mean() for v in value)
            else:
                raise TypeError(f'{name} is not a tensor or list of tensors')
        loss = sum(v for k, v in log_vars.items() if 'loss' in k)
        log_vars['loss'] = loss
        stacked = torch.stack([v.detach().float() for v in log_vars.values()])
        if dist.is_available() and dist.is_initialized():
            stacked = stacked / dist.get_world_size()
            dist.all_reduce(stacked)                       # one message instead of one per scalar
        return loss, DeferredLogVars(log_vars.keys(), stacked)
