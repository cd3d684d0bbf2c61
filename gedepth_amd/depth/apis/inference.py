"""Depth for one camera frame (role of depth/apis/inference.py:12-105: ``init_depther`` / ``inference_depther``).

The reference's ``inference_depther`` replaces ``LoadImageFromFile`` by a plain ``LoadImage``, so the two ground-embedding channels
never reach a GEDepth model.  Here a frame takes the configured KITTI test protocol — LoadImageFromFile(USEPE) -> KBCrop ->
MultiScaleFlipAug(RandomFlip, Normalize) -> ``aug_test`` — on the device, through ``DepthInferencer``:

  1. the uint8 BGR frame is uploaded from pinned memory (non-blocking, on the engine's stream);
  2. ``ge_infer_front`` (csrc/infer.hip) writes both flip views, normalised, into a static (2, 5, 352, 1216) buffer;
  3. ``model.encode_decode`` runs the two views as ONE batch-2 forward (clamped and rescaled, as ``inference`` does);
  4. ``ge_tta_merge`` forms (view 0 + mirror(view 1)) / 2 into a static (1, 352, 1216) output, in aug_test's order;
  5. the output is copied to the host (``to_host=False``: it stays in the static device buffer, for ``single_gpu_test(device_eval=True)``).

After two eager calls, steps 3-4 are captured in a hipGraph and replayed for every later frame.  KB crop makes the forward's shape
constant, so frames of every KITTI size share one graph; only the front end's arguments change, and it stays outside the graph.

A DDAD config (``front_spec(cfg)['protocol'] == 'ddad'``) takes LoadDDADImageFromFile(USEPE, USE_DYNAMIC_PE) -> DDADResize(shape, depth=False)
-> MultiScaleFlipAug(flip=False, Normalize) -> ``simple_test`` instead: ``ge_infer_front_ddad`` writes the one view into a static
(1, 5, Hd, Wd) buffer, the camera's height goes into a static (1,) tensor (the adaptive ground embedding reads it through a device pointer,
so a replayed graph follows it) and the forward's (1, Hd, Wd) map is the output.  The frame's camera names the ground depth
(``<pe_root>/<camera>/ddad_pe.npz``) and the height: the ``camera=`` argument, else the image path's parent directory.
``_KITTIFront`` / ``_DDADFront`` hold what the protocols do differently per frame; ``engine_for`` keeps a model's engines for every caller.
``inference_depther(batch=F)`` runs F KITTI frames per forward instead (apis/batch_inference.py); ``batch=1``, the default, is this engine.
F DDAD frames per forward: ``BatchDDADInferencer`` there (``engine_for(model, bf16, batch=F)``), which ``inference_depther`` does not reach.
"""
import gc
import os.path as osp

import numpy as np
import torch
from PIL import Image

from ... import kernels as K
from ...ground_kernels import PLANES
from ...mmrt.checkpoint import load_checkpoint
from ...mmrt.config import Config
from ..datasets.pipelines import loading    # _DDAD_CAMERA_HEIGHT is read through the module at every use, so a changed table is seen
from ..models import build_depther
from ..utils.pinned import PinnedUpload

__all__ = ['init_depther', 'inference_depther', 'inference_point_cloud', 'inference_ground', 'inference_scene_cloud', 'inference_error_map', 'inference_prior_sweep', 'DepthInferencer',
           'kitti_front_spec', 'ddad_front_spec', 'front_spec', 'SCENE_LAYERS']

# test-time transforms of MultiScaleFlipAug the device front end restates (ImageToTensor / Collect are layout only)
_FRONT_TRANSFORMS = ('RandomFlip', 'Normalize', 'ImageToTensor', 'Collect')
_PROTOCOL = 'LoadImageFromFile(USEPE) -> KBCrop -> MultiScaleFlipAug(RandomFlip, Normalize)'
_DDAD_TRANSFORMS = ('Normalize', 'ImageToTensor', 'Collect')
_DDAD_PROTOCOL = ('LoadDDADImageFromFile(USEPE, USE_DYNAMIC_PE) -> DDADResize(shape, depth=False) -> '
                  'MultiScaleFlipAug(flip=False, Normalize)')


def init_depther(config, checkpoint=None, device='cuda:0'):
    """Build a depther from a config file path or ``Config``; load ``checkpoint`` (mmcv layout) when given; the model keeps the config
    as ``model.cfg``, sits on ``device`` and is in eval mode."""
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError(f'config must be a filename or Config object, but got {type(config)}')
    config.model.pretrained = None
    config.model.train_cfg = None
    model = build_depther(config.model, test_cfg=config.get('test_cfg'))
    if checkpoint is not None:
        ckpt = load_checkpoint(model, checkpoint, map_location='cpu')
        meta = ckpt.get('meta') or {}
        for key in ('CLASSES', 'PALETTE'):
            if key in meta:
                setattr(model, key, meta[key])
    model.cfg = config
    model.to(device)
    model.eval()
    return model


def _aug_spec(aug, allowed, front_end, name, steps):
    """Both protocols' MultiScaleFlipAug -> ``(inner transform types, the spec fields of its Normalize)``; errors in the caller's words."""
    inner = [t['type'] for t in aug['transforms']]
    for t in inner:
        if t not in allowed:
            raise NotImplementedError(f'MultiScaleFlipAug transform {t}: no {front_end} for it ({steps})')
    norm = next((t for t in aug['transforms'] if t['type'] == 'Normalize'), None)
    if norm is None:
        raise NotImplementedError(f'MultiScaleFlipAug without Normalize: not the {name} protocol {steps}')
    # Normalize holds mean / std as float32 and widens them to float64 (imageops.imnormalize)
    return inner, dict(mean=[float(np.float32(v)) for v in norm['mean']], std=[float(np.float32(v)) for v in norm['std']],
                       to_rgb=bool(norm.get('to_rgb', True)), depth_scale=float(norm.get('depth_scale', 200)))


def kitti_front_spec(cfg):
    """The parameters of the configured test pipeline the device front end needs; ``NotImplementedError`` for any other protocol."""
    pipeline = cfg.data.test.pipeline
    types = [t['type'] for t in pipeline]
    load = next((t for t in pipeline if t['type'] == 'LoadImageFromFile'), None)
    kb = next((t for t in pipeline if t['type'] == 'KBCrop'), None)
    aug = next((t for t in pipeline if t['type'] == 'MultiScaleFlipAug'), None)
    other = [t for t in types if t not in ('LoadImageFromFile', 'LoadKITTICamIntrinsic', 'KBCrop', 'MultiScaleFlipAug')]
    if other:
        raise NotImplementedError(f'test pipeline step(s) {", ".join(other)}: no device front end for them (inference_depther '
                                  f'implements the KITTI protocol {_PROTOCOL})')
    if load is None or kb is None or aug is None or not load.get('USEPE', False):
        raise NotImplementedError(f'test pipeline {types}: inference_depther implements the KITTI protocol {_PROTOCOL} only')
    if load.get('LOAD_DYNAMIC_PE', False):
        raise NotImplementedError('LoadImageFromFile(LOAD_DYNAMIC_PE=True): no device front end for it')
    inner, common = _aug_spec(aug, _FRONT_TRANSFORMS, 'device front end', 'KITTI', _PROTOCOL)
    directions = aug.get('flip_direction', 'horizontal')
    directions = directions if isinstance(directions, list) else [directions]
    flip = bool(aug.get('flip', False)) and 'RandomFlip' in inner
    if aug.get('img_ratios') is not None or (flip and directions != ['horizontal']):
        raise NotImplementedError('multi-scale or vertical-flip test-time augmentation: no device front end for it')
    return dict(common, height=int(kb.get('height', 352)), width=int(kb.get('width', 1216)), views=2 if flip else 1,
                pe_max=float(load.get('pe_max', 200)), pe_root=load.get('pe_root'))


def ddad_front_spec(cfg):
    """The parameters of the configured DDAD test pipeline the device front end needs; ``NotImplementedError``, naming the step, for
    anything but ``_DDAD_PROTOCOL``."""
    pipeline = cfg.data.test.pipeline
    types = [t['type'] for t in pipeline]
    other = [t for t in types if t not in ('LoadDDADImageFromFile', 'DDADResize', 'MultiScaleFlipAug')]
    if other:
        raise NotImplementedError(f'test pipeline step(s) {", ".join(other)}: no DDAD device front end for them (it implements '
                                  f'{_DDAD_PROTOCOL})')
    if types != ['LoadDDADImageFromFile', 'DDADResize', 'MultiScaleFlipAug']:
        raise NotImplementedError(f'test pipeline {types}: the DDAD device front end implements {_DDAD_PROTOCOL} only')
    load, resize, aug = pipeline
    # without USE_DYNAMIC_PE the host builds a 4-channel image whose ground depth DDADResize area-averages, and no camera height
    if not load.get('USEPE', False) or not load.get('USE_DYNAMIC_PE', False):
        raise NotImplementedError('LoadDDADImageFromFile without USEPE=True, USE_DYNAMIC_PE=True: no device front end for it')
    if load.get('to_float32', False):
        raise NotImplementedError('LoadDDADImageFromFile(to_float32=True): no device front end for it')
    if resize.get('depth', True):
        raise NotImplementedError('DDADResize(depth=True): the test protocol resizes no depth; no device front end for it')
    _, common = _aug_spec(aug, _DDAD_TRANSFORMS, 'DDAD device front end', 'DDAD', _DDAD_PROTOCOL)
    if aug.get('flip', False):
        raise NotImplementedError('MultiScaleFlipAug(flip=True): no flip test-time augmentation on the DDAD device front end')
    if aug.get('img_ratios') is not None:
        raise NotImplementedError('MultiScaleFlipAug(img_ratios=...): no multi-scale test-time augmentation on the DDAD device front end')
    shape = tuple(int(v) for v in resize['shape'])
    return dict(common, protocol='ddad', height=shape[0], width=shape[1], views=1,
                pe_max=250.0,                                          # LoadDDADImageFromFile's constant
                pe_root=load.get('pe_root') if load.get('pe_root') is not None else osp.join('data', 'DDAD', 'pe_public_debug'))


def front_spec(cfg):
    """``ddad_front_spec`` for a pipeline with a DDAD step, else ``kitti_front_spec``, with ``protocol`` = 'ddad' / 'kitti'."""
    types = [t['type'] for t in cfg.data.test.pipeline]
    if 'LoadDDADImageFromFile' in types or 'DDADResize' in types:
        return ddad_front_spec(cfg)
    return dict(kitti_front_spec(cfg), protocol='kitti')


def _ddad_camera(camera, path):
    """The frame's camera: ``camera``, else the image path's parent directory (as LoadDDADCamIntrinsic takes it); None when neither names
    one.  A ``camera`` argument that is not a DDAD camera with a known height is a ``ValueError``."""
    known = loading._DDAD_CAMERA_HEIGHT
    if camera is not None:
        if camera not in known:
            raise ValueError(f'camera {camera!r}: the cameras with a known height are {", ".join(sorted(known))}')
        return camera
    if isinstance(path, str):
        parent = osp.basename(osp.dirname(path))
        if parent in known:
            return parent
    return None


def _img_prefix(cfg):
    test = cfg.data.test
    img_dir, root = test.get('img_dir'), test.get('data_root')
    if img_dir is None:
        return root
    return img_dir if root is None or osp.isabs(img_dir) else osp.join(root, img_dir)


def _pe_file(spec, prefix, path):
    """``<pe_root or img prefix>/<date>/pe/pe_165.npy`` for an image path inside the test tree, as LoadImageFromFile finds it; else None."""
    if not isinstance(path, str) or prefix is None:
        return None
    rel = osp.relpath(osp.abspath(path), osp.abspath(prefix))
    if rel.startswith('..') or osp.isabs(rel):
        return None
    root = spec['pe_root'] if spec['pe_root'] is not None else prefix
    npy = osp.join(root, rel.split(osp.sep)[0], 'pe', 'pe_165.npy')
    return npy if osp.isfile(npy) else None


_NO_PE = ('no ground depth for this frame: pass pe= (the raw (H, W) map), calib=(calib_cam_to_cam.txt, calib_velo_to_cam.txt), or an '
          'image path inside cfg.data.test.data_root/img_dir whose <date>/pe/pe_165.npy exists')


def _decode(img):
    """A path (decoded as the host LoadImageFromFile does: PIL, RGB -> BGR) or an (H, W, 3) uint8 BGR array -> contiguous uint8 BGR."""
    if isinstance(img, str):
        return np.ascontiguousarray(np.asarray(Image.open(img).convert('RGB'))[..., ::-1])
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise TypeError(f'img must be a path or an (H, W, 3) uint8 BGR array, got {a.shape} {a.dtype}')
    return np.ascontiguousarray(a)


class _KITTIFront:
    """KITTI's own part of a frame's way through ``DepthInferencer``; no state, the engine is handed in."""

    def frame(self, eng, H, W, path, camera):
        """The frame's argument errors, before any device work -> ``(camera, ori_shape of the metas)``; DDAD's also sets ``eng.frame_size``."""
        s = eng.spec
        if H < s['height'] or W < s['width']:
            raise ValueError(f'frame {(H, W)} is smaller than the KB crop {(s["height"], s["width"])}')
        return None, (s['height'], s['width'], 5)

    def fill(self, eng, bgr, path, cam, pe, calib, cam_height):
        """On the engine's stream, outside its graph: ground depth, upload, front kernel into ``static_in``; returns ``last_frame``."""
        s = eng.spec
        H, W = bgr.shape[:2]
        top, left = int(H - s['height']), int((W - s['width']) / 2)       # KBCrop
        raw = eng.last_ground_depth = eng.ground_depth(H, W, path, pe, calib, cam_height)       # kept for ``scene_points``
        dev = eng.upload(bgr)
        K.infer_front(dev, raw, eng.static_in, top, left, s['mean'], s['std'], s['to_rgb'], s['pe_max'], s['depth_scale'])
        return dev, top, left


class _DDADFront:
    """DDAD's: the camera names ground depth and height, the frames of one engine have one size."""

    def frame(self, eng, H, W, path, camera):
        s = eng.spec
        cam = _ddad_camera(camera, path)
        if cam is None:
            raise ValueError(f'no camera for this frame: pass camera= (one of {", ".join(sorted(loading._DDAD_CAMERA_HEIGHT))}) or an '
                             'image path whose parent directory is the camera name')
        if H < s['height'] or W < s['width']:
            raise ValueError(f'frame {(H, W)} is smaller than DDADResize\'s shape {(s["height"], s["width"])}')
        if eng.frame_size is not None and eng.frame_size != (H, W):
            raise ValueError(f'frame {(H, W)}: this engine takes frames of {eng.frame_size} (reset() to change)')
        eng.frame_size = (H, W)
        return cam, (H, W, 5)                        # LoadDDADImageFromFile: ori_shape = the frame's

    def fill(self, eng, bgr, path, cam, pe, calib, cam_height):
        s = eng.spec
        raw = eng.ground_depth_ddad(cam, *bgr.shape[:2], pe)
        dev = eng.upload(bgr)
        K.infer_front_ddad(dev, raw, eng.static_in, s['mean'], s['std'], s['to_rgb'], s['pe_max'], s['depth_scale'])
        eng.static_height.fill_(float(loading._DDAD_CAMERA_HEIGHT[cam]))


def _config_of(model):
    """``(front_spec, image prefix)`` of ``model.cfg``; host work only, so argument errors can be read off it before any device work."""
    cfg = getattr(model, 'cfg', None)
    if cfg is None:
        raise ValueError('model.cfg is missing: build the model with init_depther (or set model.cfg to its Config)')
    return front_spec(cfg), _img_prefix(cfg)


class DepthInferencer:
    """The flip-TTA engine of one model and precision (module docstring).  ``captures`` counts hipGraph captures and ``replays`` their replays; ``reset()`` drops
    the graphs and zeroes both.

    A capture is keyed by the precision and the ``kernel_variant`` of every module that has one.  It bakes in the addresses of the
    parameters, buffers and static tensors: parameters must be updated IN PLACE (``load_state_dict``, ``param.data.copy_``) for a replay to
    see them; replacing a parameter tensor needs ``reset()``.  Host-side heuristics evaluated at capture time (the cross-attention's query
    order) are frozen into the graph as in mmrt/graph.py; results do not depend on them.  ``front``: the protocol's own part of a frame."""

    WARMUP = 2

    def __init__(self, model, bf16=False, config=None):
        self.model, self.bf16 = model, bool(bf16)
        self.spec, self.prefix = config or _config_of(model)
        self.ddad = self.spec['protocol'] == 'ddad'
        self.front = _DDADFront() if self.ddad else _KITTIFront()
        self.device = next(model.parameters()).device
        s = self.spec
        self.static_in = torch.empty(s['views'], 5, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self.static_out = torch.empty(1, s['height'], s['width'], device=self.device, dtype=torch.float32)
        # DDAD: the camera height, filled per frame outside the graph; ground_embed_adaptive reads it through its device pointer
        self.static_height = torch.zeros(1, device=self.device, dtype=torch.float32) if self.ddad else None
        self._forward_kw = dict(height=self.static_height) if self.ddad else {}      # no ``test`` key: _height takes the tensor as it is
        self.stream = torch.cuda.Stream(self.device)
        self._staging = PinnedUpload()
        self._pe = {}
        self.last_frame = None                   # KITTI: (device uint8 BGR frame, top, left) of the last call, for ``points``
        self.last_ground_depth = None            # KITTI: the raw (H, W) f32 ground depth the last call's front end was given
        self.last_gt = None                      # the (H, W) uint16 ground truth ``scene_points`` last uploaded
        self._gt_staging = PinnedUpload()
        self.static_ground = self.static_ground_valid = None      # (4, H, W) f32 / (H, W) u8 of ``ground_maps``, allocated at its first call
        self.reset()

    def reset(self):
        """Drop every captured graph (and its memory pool) and the warm-up counts."""
        self.graphs, self.calls, self.captures, self.replays = {}, {}, 0, 0
        self.frame_size = None                   # DDAD: the (H, W) of the frames this engine has taken

    @property
    def last_frames(self):
        """``[last_frame]`` or None: what the batched engines keep per slot under this name, so a loop reads one name from any engine."""
        return None if self.last_frame is None else [self.last_frame]

    @property
    def last_ground_depths(self):
        """``[last_ground_depth]`` or None, as ``last_frames``."""
        return None if self.last_ground_depth is None else [self.last_ground_depth]

    # ---- ground depth
    def _cache(self, key, make):
        if key not in self._pe:
            if len(self._pe) >= 16:
                self._pe.clear()
            self._pe[key] = make()
        return self._pe[key]

    def ground_depth(self, H, W, path=None, pe=None, calib=None, cam_height=1.65):
        """Raw (H, W) f32 ground depth on the device: ``pe``, else ``calib``, else ``<date>/pe/pe_165.npy`` of the test tree."""
        if pe is not None:
            t = torch.as_tensor(pe)
            if tuple(t.shape) != (H, W):
                raise ValueError(f'pe has shape {tuple(t.shape)}, the frame is {(H, W)}')
            return t.to(self.device, torch.float32, non_blocking=True).contiguous()
        if calib is not None:
            from ..datasets.gpu_pipeline import ground_depth_from_calibration
            cam, velo = (osp.abspath(p) for p in calib)
            return self._cache(('calib', cam, velo, float(cam_height), H, W),
                               lambda: ground_depth_from_calibration(cam, velo, H, W, cam_height, self.device).contiguous())
        npy = _pe_file(self.spec, self.prefix, path)
        if npy is None:
            raise ValueError(_NO_PE)
        return self._cache(('npy', npy, H, W), lambda: self._load_pe(npy, np.load(npy), H, W))

    def ground_depth_ddad(self, camera, H, W, pe=None):
        """Raw (H, W) f32 ground depth of ``camera`` on the device: ``pe``, else ``<pe_root>/<camera>/ddad_pe.npz['pe']`` (once per camera)."""
        if pe is not None:
            return self.ground_depth(H, W, pe=pe)
        npz = osp.join(self.spec['pe_root'], camera, 'ddad_pe.npz')
        return self._cache(('ddad', npz, H, W), lambda: self._load_pe(npz, np.load(npz)['pe'], H, W))

    def _load_pe(self, file, a, H, W):
        a = a.astype(np.float32)
        if a.shape != (H, W):
            raise ValueError(f'{file} has shape {a.shape}, the frame is {(H, W)}')
        return torch.from_numpy(a).to(self.device).contiguous()

    # ---- one frame
    def _key(self, ground=False):
        key = (self.bf16,) + tuple(m.kernel_variant for m in self.model.modules() if hasattr(m, 'kernel_variant'))
        return key + ('ground',) if ground else key

    def _metas(self, filename, shape, ori_shape):
        s = self.spec
        norm = dict(mean=np.float32(s['mean']), std=np.float32(s['std']), to_rgb=s['to_rgb'])
        return [dict(filename=filename, ori_filename=filename, ori_shape=ori_shape, img_shape=tuple(shape) + (5,),
                     pad_shape=tuple(shape) + (5,), scale_factor=1.0, flip=bool(v), flip_direction='horizontal', img_norm_cfg=norm)
                for v in range(s['views'])]

    def _body(self, metas, ground=False):
        model = self.model
        model.keep_ground_lr = ground                # the forward keeps the two ground necks' low-resolution outputs for ge_ground_maps
        try:
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.bf16):
                pred = model.encode_decode(self.static_in, metas, rescale=True, **self._forward_kw)
            lr, model.ground_lr = model.ground_lr, None
        finally:
            model.keep_ground_lr = False
        pred = pred.float().contiguous()
        if self.spec['views'] == 2:
            K.tta_merge(pred, self.static_out)
        else:
            self.static_out.copy_(pred[0])
        if ground:
            if lr is None:
                raise NotImplementedError('ground_maps: the model has no ground embedding (no pe_mask_neck)')
            # the model's own arguments: its depth_scale (the configs set it to the pipeline's), the vanilla branch's constant 200
            K.ground_maps(*lr, self.static_in, self.static_height, model.depth_scale, 200.0, flip=self.spec['views'] == 2,
                          out=self.static_ground, valid=self.static_ground_valid)

    def _run(self, key, graph, body):
        """``body()`` on the current (the engine's) stream: eagerly for the first ``WARMUP`` calls under ``key`` (and whenever ``graph``
        is false), then captured once in a hipGraph and replayed from then on."""
        g = self.graphs.get(key) if graph else None
        if graph and g is None and self.calls.get(key, 0) >= self.WARMUP:
            g = torch.cuda.CUDAGraph()
            # The cycle collector must not run inside the capture (torch.cuda.graph does not collect before it by default): a dead
            # cycle it frees there (a model and the engine it kept, with pinned buffer, events and device tensors) makes runtime
            # calls that a capturing thread may not make, and an error raised inside a destructor ends the process.  It runs again
            # right after the capture.
            collecting = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g, stream=self.stream):
                    body()
            finally:
                if collecting:
                    gc.enable()
            self.graphs[key] = g
            self.captures += 1
        if g is not None:
            g.replay()
            self.replays += 1
        else:
            body()
            if graph:
                self.calls[key] = self.calls.get(key, 0) + 1

    def upload(self, bgr):
        """Host uint8 frame -> device, through a reused pinned buffer and a non-blocking copy on the current stream (``PinnedUpload``)."""
        return self._staging(bgr, self.device)

    def __call__(self, img, pe=None, calib=None, cam_height=1.65, graph=True, to_host=True, camera=None):
        """One frame -> its (1, 352, 1216) float32 map (DDAD: (1, Hd, Wd) of DDADResize's shape): a fresh host array, or with
        ``to_host=False`` the static device buffer ``static_out`` itself, without synchronising: valid until the next call, and ordered on
        ``self.stream`` (the caller's current stream waits for it, as always).  ``camera`` (DDAD): the frame's camera, else the image
        path's parent directory; ``calib`` / ``cam_height`` belong to the KITTI protocol."""
        return self._frame(img, pe, calib, cam_height, graph, to_host, camera, False)

    def ground_maps(self, img, pe=None, calib=None, cam_height=1.65, graph=True, to_host=True, camera=None):
        """One frame -> a dict with its map and the ground embedding's own maps, merged over the views as the map is: ``depth``
        (1, H, W) as ``__call__`` returns it; ``attention`` (the ground attention y: the depth is ``relu(c) * (1 - y) + ground_term +
        min_depth``), ``ground_term`` (the ground's share of that sum) and ``ground_depth`` (the slope-adjusted ground plane in metres,
        averaged over the views where it is valid, 0 where none is), each (H, W) float32; ``slope_deg`` (H, W), the predicted road slope
        in degrees, for an adaptive model only; ``valid`` (H, W) uint8, the number of views with a valid ground depth.  Arguments as in
        ``__call__``.  ``ge_ground_maps`` (include/gedepth_ground.h) runs right after the merge, inside the captured graph, on the
        low-resolution outputs of the two ground necks; the capture is keyed apart from ``__call__``'s, so the two modes keep one graph
        each.  ``to_host=False``: views of the static buffers ``static_out`` / ``static_ground`` / ``static_ground_valid`` (allocated at
        the first call of this method), valid until the next call and ordered on ``self.stream``."""
        return self._frame(img, pe, calib, cam_height, graph, to_host, camera, True)

    def _frame(self, img, pe, calib, cam_height, graph, to_host, camera, ground, bgr=None):
        bgr = _decode(img) if bgr is None else bgr           # ``bgr``: ``img`` as a caller has decoded it already
        H, W = bgr.shape[:2]
        path = img if isinstance(img, str) else None
        cam, ori_shape = self.front.frame(self, H, W, path, camera)
        metas = self._metas(path, (H, W), ori_shape)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.last_frame = self.front.fill(self, bgr, path, cam, pe, calib, cam_height)     # per frame: outside the graph
            if ground and self.static_ground is None:
                s = self.spec
                self.static_ground = torch.empty(4, s['height'], s['width'], device=self.device, dtype=torch.float32)
                self.static_ground_valid = torch.empty(s['height'], s['width'], device=self.device, dtype=torch.uint8)
            self._run(self._key(ground), graph, lambda: self._body(metas, ground))
            # to_host: synchronises the engine's stream; a fresh host array per frame
            if ground:
                out = dict(zip(PLANES, self.static_ground), depth=self.static_out, valid=self.static_ground_valid)
                if not self.model.dynamic_pe_neck_FLAGS:
                    del out['slope_deg']
                if to_host:
                    out = {k: v.cpu().numpy() for k, v in out.items()}
            else:
                out = self.static_out.cpu().numpy() if to_host else self.static_out
        cur.wait_stream(self.stream)
        return out

    def points(self, img, pe=None, calib=None, cam_height=1.65, graph=True, K=None, ground=False, **cloud_kw):
        """One frame -> the coloured points of its map, ``(records, count)`` device tensors as ``depth.utils.depth_to_points`` returns
        them for a CUDA map, without synchronising.  The frame runs as in ``__call__`` with ``to_host=False``; ``ge_depth_points`` then
        reads ``static_out``, the frame uploaded for this call and its KB-crop offsets on ``self.stream``, outside the captured graph (the
        capture and its key are those of ``__call__``).  Intrinsics: ``kitti_intrinsics(img, calib, K, the test tree)``, in frame
        coordinates, shifted by the crop (``cx - left``, ``cy - top``).  ``ground``: run the frame as ``ground_maps`` does instead (its
        graph; ``static_ground`` holds the frame's maps afterwards): the points need ``static_out`` and ``last_frame`` only, which both
        modes fill.  ``cloud_kw``: ``min_depth`` / ``max_depth`` (default: the decode head's), ``row0``, ``step``, ``alpha``."""
        if self.ddad:
            raise NotImplementedError(_DDAD_NO_POINTS)
        from ...kernels import depth_points                  # the module's ``K`` is this method's intrinsics argument
        from ..utils.point_cloud import kitti_intrinsics
        fx, fy, cx, cy = kitti_intrinsics(img if isinstance(img, str) else None, calib, K, self.prefix)     # errors before any device work
        head = self.model.decode_head
        cloud_kw.setdefault('min_depth', head.min_depth)
        cloud_kw.setdefault('max_depth', head.max_depth)
        depth = self.ground_maps(img, pe, calib, cam_height, graph, to_host=False)['depth'] if ground else \
            self(img, pe, calib, cam_height, graph, to_host=False)
        dev, top, left = self.last_frame
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            out = depth_points(depth, fx, fy, cx - left, cy - top, dev, top, left, **cloud_kw)
        cur.wait_stream(self.stream)
        return out

    def scene_points(self, img, gt=None, layers=None, pe=None, calib=None, cam_height=1.65, graph=True, K=None, gt_scale=256.0, **cloud_kw):
        """One frame -> the scene cloud of its map (role of the reference's visualize_point-cloud_kitti_gt_pe_pred.py):
        ``(records, counts)`` device tensors as ``kernels.scene_points`` returns them, without synchronising.  The layers, always in the
        order of ``SCENE_LAYERS`` whatever order ``layers`` names them in: ``'prediction'``, ``static_out`` coloured from the frame;
        ``'ground'`` (255, 0, 0), the raw ground depth this frame's front end was given, in the KB-crop window; ``'gt'`` (0, 255, 0),
        ``gt`` — a 16-bit PNG path or an (H, W) uint16 array of the frame's size, uploaded through a pinned buffer on the engine's
        stream and divided by ``gt_scale`` in the kernel — in the KB-crop window; ``'adjusted'`` (0, 0, 255), the ``ground_depth`` plane
        of ``static_ground``.  ``layers=None``: all of them, without ``'gt'`` when ``gt`` is None.  The frame runs as ``ground_maps`` with
        ``to_host=False`` when ``'adjusted'`` is among the layers and as ``__call__`` otherwise (their captures and keys); the kernel
        launches on ``self.stream`` outside the graph.  Intrinsics as in ``points``.  ``cloud_kw``: ``min_depth`` / ``max_depth``
        (default: the decode head's), shared by all layers, ``row0``, ``step``, ``alpha``.  With ``min_depth > 0`` the pixels of the
        ``adjusted`` plane without a valid ground depth (0) and the ground truth's pixels without a LiDAR return (0) drop out."""
        if self.ddad:
            raise NotImplementedError(_DDAD_NO_POINTS)
        from ...kernels import SceneLayer, scene_points            # the module's ``K`` is this method's intrinsics argument
        from ..utils.point_cloud import kitti_intrinsics
        names = _scene_layer_names(layers, gt)                       # every argument error before any device work
        fx, fy, cx, cy = kitti_intrinsics(img if isinstance(img, str) else None, calib, K, self.prefix)
        bgr = _decode(img)
        H, W = bgr.shape[:2]
        self.front.frame(self, H, W, None, None)
        raw_gt = _scene_gt(gt, H, W) if 'gt' in names else None
        head = self.model.decode_head
        dmin, dmax = float(cloud_kw.pop('min_depth', head.min_depth)), float(cloud_kw.pop('max_depth', head.max_depth))
        unknown = set(cloud_kw) - {'row0', 'step', 'alpha'}
        if unknown:
            raise TypeError(f'scene_points: unknown argument(s) {", ".join(sorted(unknown))}')
        s = self.spec
        self._frame(img, pe, calib, cam_height, graph, False, None, 'adjusted' in names, bgr)
        dev, top, left = self.last_frame
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            made = []
            for name in names:
                kw = dict(min_depth=dmin, max_depth=dmax, colour=_SCENE_COLOURS[name])
                if name == 'prediction':
                    made.append(SceneLayer(self.static_out[0], **kw))
                elif name == 'ground':
                    made.append(SceneLayer(self.last_ground_depth, top=top, left=left, **kw))
                elif name == 'gt':
                    self.last_gt = self._gt_staging(raw_gt, self.device)
                    made.append(SceneLayer(self.last_gt, 'u16', top=top, left=left, scale=gt_scale, **kw))
                else:
                    made.append(SceneLayer(self.static_ground[PLANES.index('ground_depth')], **kw))
            out = scene_points(made, fx, fy, cx - left, cy - top, s['height'], s['width'], dev, top, left, **cloud_kw)
        cur.wait_stream(self.stream)
        return out

    def error_map(self, img, gt, tau=0.05, radius=1, background=1, pe=None, calib=None, cam_height=1.65, graph=True, to_host=True, rect=None):
        """One frame and its ground truth -> ``(image (352, 1216, 3) uint8 BGR, err (352, 1216) float32)``: every LiDAR return painted
        with the band of its abs-rel error over the frame's own pixels, and the error plane itself (include/gedepth_error.h;
        ``kernels.error_image``).  ``gt``: a 16-bit PNG path or an (H, W) uint16 array of the frame's size, uploaded as ``scene_points``
        uploads it; ``tau`` in (0, 1]: the abs-rel error of the middle threshold (0.05: red from 5 %); ``radius`` 0 .. 3: a return is
        drawn (2 radius + 1) pixels wide, the worst return winning; ``background``: 0 the frame, 1 the frame halved, 2 black;
        ``rect=(r0, r1, c0, c1)``: the rows and columns of the crop whose returns count (None: all of it).  The depth limits are the decode
        head's, the ground truth is divided by 256.  The frame runs as in ``__call__`` with ``to_host=False`` (its capture and key);
        ``ge_error_image`` then reads ``static_out``, the frame uploaded for this call and its KB-crop offsets on ``self.stream``, outside
        the captured graph.  ``to_host=False``: device tensors, without synchronising."""
        if self.ddad:
            raise NotImplementedError('error_map on a DDAD engine: the DDAD ground truth is a float map at another resolution and DDADResize '
                                      'leaves no uint8 frame at the map\'s size; the error images are built for the KITTI protocol')
        from ...error_kernels import error_image, paint_args
        tau, radius, background = paint_args(tau, radius, background)           # every argument error before any device work
        s = self.spec
        rect = (0, s['height'], 0, s['width']) if rect is None else tuple(int(v) for v in rect)
        if len(rect) != 4 or not (0 <= rect[0] <= s['height'] and 0 <= rect[1] <= s['height'] and 0 <= rect[2] <= s['width']
                                  and 0 <= rect[3] <= s['width']):
            raise ValueError(f'rect {rect} is not (r0, r1, c0, c1) inside the {(s["height"], s["width"])} crop')
        bgr = _decode(img)
        H, W = bgr.shape[:2]
        self.front.frame(self, H, W, None, None)
        raw_gt = _scene_gt(gt, H, W)
        head = self.model.decode_head
        self._frame(img, pe, calib, cam_height, graph, False, None, False, bgr)
        dev, top, left = self.last_frame
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            self.last_gt = self._gt_staging(raw_gt, self.device)
            out, err = error_image(self.static_out[0], self.last_gt, dev, top, left, rect, 256.0, float(head.min_depth), float(head.max_depth),
                                   tau, radius, background)
            if to_host:
                out, err = out.cpu().numpy(), err.cpu().numpy()
        cur.wait_stream(self.stream)
        return out, err


SCENE_LAYERS = ('prediction', 'ground', 'gt', 'adjusted')          # the reference's concatenation order
_SCENE_COLOURS = {'prediction': None, 'ground': (255, 0, 0), 'gt': (0, 255, 0), 'adjusted': (0, 0, 255)}


def _scene_layer_names(layers, gt):
    """The layers of a scene cloud in ``SCENE_LAYERS``' order; an unknown name, an empty list or ``'gt'`` without ``gt`` is a ``ValueError``."""
    if layers is None:
        return [n for n in SCENE_LAYERS if n != 'gt' or gt is not None]
    asked = [layers] if isinstance(layers, str) else list(layers)
    unknown = [n for n in asked if n not in SCENE_LAYERS]
    if unknown:
        raise ValueError(f'unknown scene layer(s) {", ".join(map(repr, unknown))}: the layers are {", ".join(SCENE_LAYERS)}')
    if not asked:
        raise ValueError(f'no scene layer asked for: the layers are {", ".join(SCENE_LAYERS)}')
    if 'gt' in asked and gt is None:
        raise ValueError('the \'gt\' layer needs gt= (a 16-bit PNG path or an (H, W) uint16 array)')
    return [n for n in SCENE_LAYERS if n in asked]


def _scene_gt(gt, H, W, load=True):
    """``gt`` (a path, read as ``KITTIDataset.gt_raw`` reads it, or an array) -> the contiguous (H, W) uint16 array; a TypeError for another
    dtype, a ValueError for another size.  ``load=False``: the checks alone, a path's from the PNG header."""
    if isinstance(gt, str) and not load:
        with Image.open(gt) as im:
            ok, shape, what = im.mode == 'I;16', (im.size[1], im.size[0]), f'mode {im.mode}'
    else:
        raw = np.asarray(Image.open(gt)) if isinstance(gt, str) else np.asarray(gt)
        ok, shape, what = raw.dtype == np.uint16 and raw.ndim == 2, raw.shape, f'{raw.dtype} {raw.shape}'
    if not ok:
        raise TypeError(f'gt must be a 16-bit single-channel PNG or an (H, W) uint16 array, got {what}')
    if tuple(shape) != (H, W):
        raise ValueError(f'gt has shape {tuple(shape)}, the frame is {(H, W)}')
    return np.ascontiguousarray(raw) if load else None


_DDAD_NO_POINTS = ('point clouds on a DDAD engine: DDADResize feeds the network an area-resized frame that exists only normalised, so there '
                   'is no uint8 colour at the map\'s size to read; depth.utils.depth_to_points with the map, intrinsics scaled to it and '
                   'a frame the caller has resized serves DDAD maps')


def engine_for(model, bf16=False, config=None, batch=1):
    """The engine of ``model``, ``bf16`` and ``batch`` frame slots in ``model._ge_inferencers``, rebuilt when ``config`` (default
    ``_config_of(model)``) has changed.  ``batch=1``: the ``DepthInferencer`` under key ``bf16``; ``batch=F > 1``: a
    ``BatchDepthInferencer`` (apis/batch_inference.py) under key ``(bf16, F)``, for a DDAD config a ``BatchDDADInferencer``."""
    spec, prefix = config = config or _config_of(model)
    engines = model.__dict__.setdefault('_ge_inferencers', {})
    bf16 = bool(bf16)
    key = bf16 if batch == 1 else (bf16, batch)
    if key not in engines or engines[key].spec != spec or engines[key].prefix != prefix:
        if batch == 1:
            engines[key] = DepthInferencer(model, bf16, config)
        else:
            from .batch_inference import BatchDDADInferencer, BatchDepthInferencer
            engines[key] = (BatchDDADInferencer if spec['protocol'] == 'ddad' else BatchDepthInferencer)(model, batch, bf16, config)
    return engines[key]


def _per_frame(value, n, error):
    """``value`` for each of ``n`` frames: a list holds one per frame (else ``ValueError(error)``), anything else serves every frame."""
    values = value if isinstance(value, list) else [value] * n
    if len(values) != n:
        raise ValueError(error.format(n=len(values), m=n))
    return values


def inference_depther(model, img, pe=None, calib=None, cam_height=1.65, bf16=False, graph=True, camera=None, batch=1):
    """Depth for each frame of ``img`` (a path, an (H, W, 3) uint8 BGR array, or a list of these): a list with one (1, 352, 1216)
    float32 array per frame — what ``model(return_loss=False, rescale=True, **data)`` returns for that frame through the config's test
    pipeline.  The raw (H, W) ground depth at frame size comes from ``pe`` (array or device tensor; a list: one per frame), else from
    ``calib=(calib_cam_to_cam.txt, calib_velo_to_cam.txt)`` with ``cam_height`` (computed on the device, cached per calibration and
    size), else from ``<date>/pe/pe_165.npy`` of an image path inside ``cfg.data.test.data_root/img_dir``.  ``bf16``: the forward under
    bf16 autocast.  ``graph``: replay a captured hipGraph of forward + merge after two eager calls (``DepthInferencer``).

    ``batch=F`` (2 .. 8; KITTI protocol): the list runs F frames per forward through a ``BatchDepthInferencer`` (apis/batch_inference.py),
    the next batch's files decoding on a small thread pool meanwhile; the result is the same list in the same order.  The frames of a
    batch may differ in size.  Every argument error — also a frame smaller than the crop — is raised for the whole list before any
    device work.  With a DDAD config ``batch > 1`` raises ``NotImplementedError``: DDAD files run in batches through
    ``engine_for(model, bf16, batch=F).run(files)`` (``BatchDDADInferencer``, apis/batch_inference.py).

    With a DDAD config every frame needs its camera: ``camera`` (a name, or a list with one per frame), else the image path's parent
    directory.  The result is one (1, Hd, Wd) map per frame at DDADResize's shape — what ``simple_test`` returns; the ground depth comes
    from ``pe``, else from ``<pe_root>/<camera>/ddad_pe.npz``.  Without a camera: ``NotImplementedError``."""
    if batch != 1:                                                            # argument errors before any device work
        from .batch_inference import check_batch, frame_size
        check_batch(batch, _config_of(model)[0])
    imgs, pes, cams, config = _frames(model, img, pe, calib, camera)
    if batch != 1:
        spec = config[0]
        for i in imgs:
            H, W = frame_size(i)
            if H < spec['height'] or W < spec['width']:
                raise ValueError(f'frame {(H, W)} is smaller than the KB crop {(spec["height"], spec["width"])}')
        return engine_for(model, bf16, config, batch).run(imgs, pes, calib, cam_height, graph)
    eng = engine_for(model, bf16, config)
    return [eng(i, p, calib, cam_height, graph, camera=c) for i, p, c in zip(imgs, pes, cams)]


def _frames(model, img, pe, calib, camera):
    """The per-frame lists and the argument errors of ``inference_depther``, before any device work -> (imgs, pes, cams, config)."""
    imgs = img if isinstance(img, list) else [img]
    pes = _per_frame(pe, len(imgs), '{n} ground-depth maps for {m} frames')
    spec, prefix = config = _config_of(model)
    cams = _per_frame(camera, len(imgs), '{n} cameras for {m} frames')
    if spec['protocol'] == 'ddad':
        if any(cam is None for cam in [_ddad_camera(c, i) for c, i in zip(cams, imgs)]):
            raise NotImplementedError('test pipeline step(s) LoadDDADImageFromFile, DDADResize: the device front end for them needs each '
                                      f'frame\'s camera (its ground depth and its height): pass camera= (one of '
                                      f'{", ".join(sorted(loading._DDAD_CAMERA_HEIGHT))}) or an image path whose parent directory is '
                                      'the camera name')
    elif calib is None and any(p is None and _pe_file(spec, prefix, i) is None for i, p in zip(imgs, pes)):
        raise ValueError(_NO_PE)
    return imgs, pes, cams, config


def inference_ground(model, img, pe=None, calib=None, cam_height=1.65, bf16=False, graph=True, camera=None):
    """The ground embedding's maps for each frame of ``img``: a list with one dict of host arrays per frame, as
    ``DepthInferencer.ground_maps`` returns it (``depth``, ``attention``, ``ground_term``, ``ground_depth``, ``valid``, and ``slope_deg``
    for an adaptive model).  Frames, ground depth, camera, ``bf16`` and ``graph`` as in ``inference_depther``, with the same argument
    errors before any device work; ``BaseDepther.show_ground`` writes one such dict as pictures."""
    imgs, pes, cams, config = _frames(model, img, pe, calib, camera)
    eng = engine_for(model, bf16, config)
    return [eng.ground_maps(i, p, calib, cam_height, graph, camera=c) for i, p, c in zip(imgs, pes, cams)]


def sweep_slots(sweep):
    """The frame slots of the batched engine that runs ``sweep`` (a ``core.PriorSweep``): its variant count, and 2 for a sweep of the
    baseline alone (``engine_for(batch=1)`` is the single-frame engine, which has no ``sweep``)."""
    return max(int(sweep.count), 2)


def inference_prior_sweep(model, img, sweep, pe=None, calib=None, bf16=False, graph=True):
    """One frame (a path or an (H, W, 3) uint8 BGR array) under every ground prior of ``sweep`` (a ``core.PriorSweep``): a list with one
    (1, 352, 1216) float32 map per variant, in the sweep's order (``sweep.names``), the first being the map ``inference_depther`` gives the
    frame — for looking at what a calibration error does to one frame's map.  Ground depth, ``bf16`` and ``graph`` as in
    ``inference_depther`` (``calib`` with ``sweep.cam_height``), with the same argument errors before any device work; the frame runs
    through ``BatchDepthInferencer.sweep`` of ``engine_for(model, bf16, batch=V)``.  A DDAD config raises ``NotImplementedError``: the
    per-camera height also feeds the network there, so the meaning of the variants needs its own decision."""
    from ..core.evaluation import PriorSweep
    if not isinstance(sweep, PriorSweep):
        raise TypeError(f'sweep must be a depth.core.PriorSweep, got {type(sweep).__name__}')
    if isinstance(img, list):
        raise TypeError('inference_prior_sweep takes one frame (a path or an (H, W, 3) uint8 BGR array), not a list')
    spec, prefix = config = _config_of(model)                                 # argument errors before any device work
    if spec['protocol'] == 'ddad':
        raise NotImplementedError('inference_prior_sweep with a DDAD config: the prior sweep is built for the KITTI protocol (on DDAD the '
                                  'per-camera height also feeds the network, so the variants\' meaning needs its own decision)')
    if calib is None and pe is None and _pe_file(spec, prefix, img) is None:
        raise ValueError(_NO_PE)
    from .batch_inference import frame_size
    H, W = frame_size(img)
    if H < spec['height'] or W < spec['width']:
        raise ValueError(f'frame {(H, W)} is smaller than the KB crop {(spec["height"], spec["width"])}')
    return engine_for(model, bf16, config, sweep_slots(sweep)).sweep(img, sweep, pe, calib, sweep.cam_height, graph)


def inference_point_cloud(model, img, pe=None, calib=None, cam_height=1.65, bf16=False, graph=True, K=None, out_file=None, **cloud_kw):
    """The coloured point cloud of each frame of ``img`` (a path, an (H, W, 3) uint8 BGR array, or a list of these): a list with one
    ``depth.utils.POINT_DTYPE`` array per frame, from ``DepthInferencer.points`` (frames, ground depth, ``bf16`` and ``graph`` as in
    ``inference_depther``).  Intrinsics: ``K`` (3x3 or 3x4, frame coordinates), else ``P_rect_02`` of ``calib``, else the recording day's
    table for an image path inside the test tree.  ``out_file`` (a path, or a list with one per frame): the ``.ply`` files are written too
    (``depth.utils.write_ply``).  ``cloud_kw``: ``min_depth``, ``max_depth``, ``row0``, ``step``, ``alpha``.

    A DDAD config raises ``NotImplementedError`` (DDADResize: no uint8 frame at the map's size); ``depth_to_points`` serves DDAD maps."""
    from ..utils.point_cloud import kitti_intrinsics, records_to_points, write_ply
    imgs = img if isinstance(img, list) else [img]
    pes = _per_frame(pe, len(imgs), '{n} ground-depth maps for {m} frames')
    outs = _per_frame(out_file if out_file is None or isinstance(out_file, list) else [out_file], len(imgs),
                      'out_file must be a list with one path per frame ({m} frames)')
    spec, prefix = config = _config_of(model)                                 # argument errors before any device work
    if spec['protocol'] == 'ddad':
        raise NotImplementedError(_DDAD_NO_POINTS)
    if calib is None and any(p is None and _pe_file(spec, prefix, i) is None for i, p in zip(imgs, pes)):
        raise ValueError(_NO_PE)
    for i in imgs:
        kitti_intrinsics(i if isinstance(i, str) else None, calib, K, prefix)
    eng = engine_for(model, bf16, config)
    clouds = []
    for i, p, o in zip(imgs, pes, outs):
        pts = records_to_points(*eng.points(i, p, calib, cam_height, graph, K, **cloud_kw))
        if o is not None:
            write_ply(o, pts)
        clouds.append(pts)
    return clouds


def inference_scene_cloud(model, img, gt=None, layers=None, out_file=None, pe=None, calib=None, cam_height=1.65, bf16=False, graph=True, K=None,
                          **cloud_kw):
    """The scene cloud of each frame of ``img`` (a path, an (H, W, 3) uint8 BGR array, or a list of these): a list with one
    ``(points, counts)`` per frame, from ``DepthInferencer.scene_points`` — ``points`` a ``depth.utils.POINT_DTYPE`` array, the layers one
    after the other, ``counts`` an ordered ``{layer name: its number of points}``.  ``gt`` (a 16-bit PNG path or an (H, W) uint16 array; a
    list: one per frame) feeds the ``'gt'`` layer; ``layers``: names out of ``SCENE_LAYERS`` (default: all, without ``'gt'`` when there is
    no ``gt``).  Frames, ground depth, intrinsics, ``bf16`` and ``graph`` as in ``inference_point_cloud``; ``out_file`` (a path, or a list
    with one per frame): the ``.ply`` files are written too (``depth.utils.write_scene_ply``).  ``cloud_kw``: ``min_depth``, ``max_depth``,
    ``row0``, ``step``, ``alpha``, ``gt_scale``.  A DDAD config raises ``NotImplementedError``, as for ``inference_point_cloud``."""
    from ..utils.point_cloud import kitti_intrinsics, scene_records_to_points, write_scene_ply
    imgs = img if isinstance(img, list) else [img]
    pes = _per_frame(pe, len(imgs), '{n} ground-depth maps for {m} frames')
    gts = _per_frame(gt, len(imgs), '{n} ground truths for {m} frames')
    outs = _per_frame(out_file if out_file is None or isinstance(out_file, list) else [out_file], len(imgs),
                      'out_file must be a list with one path per frame ({m} frames)')
    spec, prefix = config = _config_of(model)                                 # argument errors before any device work
    if spec['protocol'] == 'ddad':
        raise NotImplementedError(_DDAD_NO_POINTS)
    names = [_scene_layer_names(layers, g) for g in gts]
    if calib is None and any(p is None and _pe_file(spec, prefix, i) is None for i, p in zip(imgs, pes)):
        raise ValueError(_NO_PE)
    from .batch_inference import frame_size
    for i, g, n in zip(imgs, gts, names):
        kitti_intrinsics(i if isinstance(i, str) else None, calib, K, prefix)
        H, W = frame_size(i)
        if H < spec['height'] or W < spec['width']:
            raise ValueError(f'frame {(H, W)} is smaller than the KB crop {(spec["height"], spec["width"])}')
        if 'gt' in n:
            _scene_gt(g, H, W, load=False)
    eng = engine_for(model, bf16, config)
    clouds = []
    for i, g, p, o, n in zip(imgs, gts, pes, outs, names):
        pts, counts = scene_records_to_points(*eng.scene_points(i, g, layers, p, calib, cam_height, graph, K, **cloud_kw), n)
        if o is not None:
            write_scene_ply(o, pts, counts)
        clouds.append((pts, counts))
    return clouds


def inference_error_map(model, img, gt, out_file=None, tau=0.05, radius=1, background=1, pe=None, calib=None, cam_height=1.65, bf16=False,
                        graph=True, rect=None):
    """The error image of each frame of ``img`` (a path, an (H, W, 3) uint8 BGR array, or a list of these) against its ground truth
    ``gt`` (a 16-bit PNG path or an (H, W) uint16 array; a list: one per frame): a list with one ``(image, err)`` per frame, from
    ``DepthInferencer.error_map`` — ``image`` (352, 1216, 3) uint8 BGR, every LiDAR return in the colour of its abs-rel error's band over
    the frame's pixels, ``err`` (352, 1216) float32, the error at the returns and -1 elsewhere.  ``tau``, ``radius``, ``background`` and
    ``rect`` as there; frames, ground depth, ``bf16`` and ``graph`` as in ``inference_depther``.  ``out_file`` (a path, or a list with one
    per frame): the pictures are written too.  Every argument error is raised for the whole list before any device work.  A DDAD config
    raises ``NotImplementedError``."""
    from ...error_kernels import paint_args
    from ..models.depther.base import _imwrite_bgr
    from .batch_inference import frame_size
    imgs = img if isinstance(img, list) else [img]
    if gt is None:
        raise ValueError('inference_error_map needs gt= (a 16-bit PNG path or an (H, W) uint16 array per frame)')
    pes = _per_frame(pe, len(imgs), '{n} ground-depth maps for {m} frames')
    gts = _per_frame(gt, len(imgs), '{n} ground truths for {m} frames')
    outs = _per_frame(out_file if out_file is None or isinstance(out_file, list) else [out_file], len(imgs),
                      'out_file must be a list with one path per frame ({m} frames)')
    spec, prefix = config = _config_of(model)                                 # argument errors before any device work
    if spec['protocol'] == 'ddad':
        raise NotImplementedError('inference_error_map with a DDAD config: the error images are built for the KITTI protocol (a uint16 '
                                  'ground truth and a uint8 frame in the KB-crop window)')
    paint_args(tau, radius, background)
    if calib is None and any(p is None and _pe_file(spec, prefix, i) is None for i, p in zip(imgs, pes)):
        raise ValueError(_NO_PE)
    for i, g in zip(imgs, gts):
        H, W = frame_size(i)
        if H < spec['height'] or W < spec['width']:
            raise ValueError(f'frame {(H, W)} is smaller than the KB crop {(spec["height"], spec["width"])}')
        _scene_gt(g, H, W, load=False)
    eng = engine_for(model, bf16, config)
    results = []
    for i, g, p, o in zip(imgs, gts, pes, outs):
        picture, err = eng.error_map(i, g, tau, radius, background, p, calib, cam_height, graph, rect=rect)
        if o is not None:
            _imwrite_bgr(picture, o)
        results.append((picture, err))
    return results
