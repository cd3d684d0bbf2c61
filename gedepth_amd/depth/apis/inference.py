"""Depth for camera frames (role of depth/apis/inference.py:12-105: ``init_depther`` / ``inference_depther``) through the frame engine
(apis/engine.py has the engine, its steps and the two test protocols it runs on the device).

``DepthInferencer`` is the engine with one slot: one frame per forward, and the one-frame products behind it — ``ground_maps`` (the ground
embedding's own maps, inside the captured graph under a key of their own), ``points``, ``scene_points`` and ``error_map`` (one kernel on
the engine's stream behind the frame, outside the graph).  With a DDAD config the frame's camera names the ground depth
(``<pe_root>/<camera>/ddad_pe.npz``) and the height: the ``camera=`` argument, else the image path's parent directory.  ``engine_for``
keeps a model's engines for every caller.  ``inference_depther(batch=F)`` runs F KITTI frames per forward through the F-slot face
(apis/batch_inference.py); ``batch=1``, the default, is this one.  F DDAD frames per forward: ``BatchDDADInferencer`` there
(``engine_for(model, bf16, batch=F)``), which ``inference_depther`` does not reach.
"""
import numpy as np
import torch
from PIL import Image

from ...ground_kernels import PLANES
from ...mmrt.checkpoint import load_checkpoint
from ...mmrt.config import Config
from ..datasets.pipelines import loading    # _DDAD_CAMERA_HEIGHT is read through the module at every use, so a changed table is seen
from ..models import build_depther
from ..utils.pinned import PinnedUpload
from .batch_inference import BatchDDADInferencer, BatchDepthInferencer, check_batch
from .engine import (FrameEngine, _config_of, _ddad_camera, _decode, _img_prefix, _per_frame, check_ground_source,  # noqa: F401
                     check_kb_crop, ddad_front_spec, frame_size, front_spec, kitti_front_spec)

__all__ = ['init_depther', 'inference_depther', 'inference_point_cloud', 'inference_ground', 'inference_scene_cloud', 'inference_error_map', 'inference_prior_sweep', 'DepthInferencer',
           'kitti_front_spec', 'ddad_front_spec', 'front_spec', 'SCENE_LAYERS']


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


class DepthInferencer(FrameEngine):
    """The engine with one slot (module docstring): the flip-TTA (KITTI) or single-view (DDAD) map of one frame per call, and the
    one-frame products.  The capture, its key and the contract that parameters are updated IN PLACE are ``FrameEngine``'s."""

    NO_CAMERA = 'no camera for this frame: pass camera= (one of {known}) or an image path whose parent directory is the camera name'

    def __init__(self, model, bf16=False, config=None):
        super().__init__(model, 1, bf16, config)
        self.last_gt = None                      # the (H, W) uint16 ground truth ``scene_points`` last uploaded
        self._gt_staging = PinnedUpload()
        self.static_ground = self.static_ground_valid = None      # (4, H, W) f32 / (H, W) u8 of ``ground_maps``, allocated at its first call

    def _public_out(self, slots):
        return slots[0]

    @property
    def last_frame(self):
        """KITTI: (device uint8 BGR frame, top, left) of the last call, slot 0 of ``last_frames``; None before it."""
        return self.last_frames[0] if self.last_frames else None

    @property
    def last_ground_depth(self):
        """KITTI: the raw (H, W) f32 ground depth the last call's front end was given, slot 0 of ``last_ground_depths``."""
        return self.last_ground_depths[0] if self.last_ground_depths else None

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
        paths, sizes = [img if isinstance(img, str) else None], [bgr.shape[:2]]
        cams, oris = self.front.check(self, sizes, paths, [camera], [pe])

        def fill():
            self.front.fill(self, [bgr], paths, cams, [pe], calib, cam_height)
            if ground and self.static_ground is None:
                s = self.spec
                self.static_ground = torch.empty(4, s['height'], s['width'], device=self.device, dtype=torch.float32)
                self.static_ground_valid = torch.empty(s['height'], s['width'], device=self.device, dtype=torch.uint8)

        def tail():                                           # to_host: synchronises the engine's stream; a fresh host array per frame
            if not ground:
                return self.static_out.cpu().numpy() if to_host else self.static_out
            out = dict(zip(PLANES, self.static_ground), depth=self.static_out, valid=self.static_ground_valid)
            if not self.model.dynamic_pe_neck_FLAGS:
                del out['slope_deg']
            return {k: v.cpu().numpy() for k, v in out.items()} if to_host else out

        return self._submit(1, fill, self._metas(paths, sizes, oris), graph, tail, ground)

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
        from ...kernels import depth_points
        from ..utils.point_cloud import kitti_intrinsics
        fx, fy, cx, cy = kitti_intrinsics(img if isinstance(img, str) else None, calib, K, self.prefix)     # errors before any device work
        head = self.model.decode_head
        cloud_kw.setdefault('min_depth', head.min_depth)
        cloud_kw.setdefault('max_depth', head.max_depth)
        self._frame(img, pe, calib, cam_height, graph, False, None, ground)
        dev, top, left = self.last_frame
        return self._after(lambda: depth_points(self.static_out, fx, fy, cx - left, cy - top, dev, top, left, **cloud_kw))

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
        from ...kernels import SceneLayer, scene_points
        from ..utils.point_cloud import kitti_intrinsics
        names = _scene_layer_names(layers, gt)                       # every argument error before any device work
        fx, fy, cx, cy = kitti_intrinsics(img if isinstance(img, str) else None, calib, K, self.prefix)
        bgr = _decode(img)
        H, W = bgr.shape[:2]
        check_kb_crop(self.spec, H, W)
        raw_gt = _scene_gt(gt, H, W) if 'gt' in names else None
        head = self.model.decode_head
        dmin, dmax = float(cloud_kw.pop('min_depth', head.min_depth)), float(cloud_kw.pop('max_depth', head.max_depth))
        unknown = set(cloud_kw) - {'row0', 'step', 'alpha'}
        if unknown:
            raise TypeError(f'scene_points: unknown argument(s) {", ".join(sorted(unknown))}')
        s = self.spec
        self._frame(img, pe, calib, cam_height, graph, False, None, 'adjusted' in names, bgr)
        dev, top, left = self.last_frame

        def cloud():
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
            return scene_points(made, fx, fy, cx - left, cy - top, s['height'], s['width'], dev, top, left, **cloud_kw)

        return self._after(cloud)

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
        check_kb_crop(s, H, W)
        raw_gt = _scene_gt(gt, H, W)
        head = self.model.decode_head
        self._frame(img, pe, calib, cam_height, graph, False, None, False, bgr)
        dev, top, left = self.last_frame

        def picture():
            self.last_gt = self._gt_staging(raw_gt, self.device)
            out, err = error_image(self.static_out[0], self.last_gt, dev, top, left, rect, 256.0, float(head.min_depth), float(head.max_depth),
                                   tau, radius, background)
            return (out.cpu().numpy(), err.cpu().numpy()) if to_host else (out, err)

        return self._after(picture)


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
            engines[key] = (BatchDDADInferencer if spec['protocol'] == 'ddad' else BatchDepthInferencer)(model, batch, bf16, config)
    return engines[key]


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
        check_batch(batch, _config_of(model)[0])
    imgs, pes, cams, config = _frames(model, img, pe, calib, camera)
    if batch != 1:
        for i in imgs:
            check_kb_crop(config[0], *frame_size(i))
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
    else:
        check_ground_source(spec, prefix, imgs, pes, calib)
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
    check_ground_source(spec, prefix, [img], [pe], calib)
    check_kb_crop(spec, *frame_size(img))
    return engine_for(model, bf16, config, sweep_slots(sweep)).sweep(img, sweep, pe, calib, sweep.cam_height, graph)


def _cloud_frames(model, img, pe, out_file, refusal):
    """What the per-frame products share: the frames, their ground depths and output files as lists, the config (a DDAD one raises
    ``NotImplementedError(refusal)``) -> ``(imgs, pes, outs, config)``."""
    imgs = img if isinstance(img, list) else [img]
    pes = _per_frame(pe, len(imgs), '{n} ground-depth maps for {m} frames')
    outs = _per_frame(out_file if out_file is None or isinstance(out_file, list) else [out_file], len(imgs),
                      'out_file must be a list with one path per frame ({m} frames)')
    config = _config_of(model)                                                # argument errors before any device work
    if config[0]['protocol'] == 'ddad':
        raise NotImplementedError(refusal)
    return imgs, pes, outs, config


def inference_point_cloud(model, img, pe=None, calib=None, cam_height=1.65, bf16=False, graph=True, K=None, out_file=None, **cloud_kw):
    """The coloured point cloud of each frame of ``img`` (a path, an (H, W, 3) uint8 BGR array, or a list of these): a list with one
    ``depth.utils.POINT_DTYPE`` array per frame, from ``DepthInferencer.points`` (frames, ground depth, ``bf16`` and ``graph`` as in
    ``inference_depther``).  Intrinsics: ``K`` (3x3 or 3x4, frame coordinates), else ``P_rect_02`` of ``calib``, else the recording day's
    table for an image path inside the test tree.  ``out_file`` (a path, or a list with one per frame): the ``.ply`` files are written too
    (``depth.utils.write_ply``).  ``cloud_kw``: ``min_depth``, ``max_depth``, ``row0``, ``step``, ``alpha``.

    A DDAD config raises ``NotImplementedError`` (DDADResize: no uint8 frame at the map's size); ``depth_to_points`` serves DDAD maps."""
    from ..utils.point_cloud import kitti_intrinsics, records_to_points, write_ply
    imgs, pes, outs, config = _cloud_frames(model, img, pe, out_file, _DDAD_NO_POINTS)
    check_ground_source(*config, imgs, pes, calib)
    for i in imgs:
        kitti_intrinsics(i if isinstance(i, str) else None, calib, K, config[1])
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
    gts = _per_frame(gt, len(img) if isinstance(img, list) else 1, '{n} ground truths for {m} frames')
    imgs, pes, outs, config = _cloud_frames(model, img, pe, out_file, _DDAD_NO_POINTS)
    names = [_scene_layer_names(layers, g) for g in gts]
    check_ground_source(*config, imgs, pes, calib)
    for i, g, n in zip(imgs, gts, names):
        kitti_intrinsics(i if isinstance(i, str) else None, calib, K, config[1])
        H, W = frame_size(i)
        check_kb_crop(config[0], H, W)
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
    if gt is None:
        raise ValueError('inference_error_map needs gt= (a 16-bit PNG path or an (H, W) uint16 array per frame)')
    gts = _per_frame(gt, len(img) if isinstance(img, list) else 1, '{n} ground truths for {m} frames')
    imgs, pes, outs, config = _cloud_frames(model, img, pe, out_file,
                                            'inference_error_map with a DDAD config: the error images are built for the KITTI protocol '
                                            '(a uint16 ground truth and a uint8 frame in the KB-crop window)')
    paint_args(tau, radius, background)
    check_ground_source(*config, imgs, pes, calib)
    for i, g in zip(imgs, gts):
        H, W = frame_size(i)
        check_kb_crop(config[0], H, W)
        _scene_gt(g, H, W, load=False)
    eng = engine_for(model, bf16, config)
    results = []
    for i, g, p, o in zip(imgs, gts, pes, outs):
        picture, err = eng.error_map(i, g, tau, radius, background, p, calib, cam_height, graph, rect=rect)
        if o is not None:
            _imwrite_bgr(picture, o)
        results.append((picture, err))
    return results
