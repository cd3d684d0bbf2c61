"""The frame engine: F frame slots (1 <= F <= 8), one stream, one captured forward, one set of static buffers.

The reference's ``inference_depther`` replaces ``LoadImageFromFile`` by a plain ``LoadImage``, so the two ground-embedding channels
never reach a GEDepth model.  Here n <= F frames take the configured test protocol on the device.  KITTI: LoadImageFromFile(USEPE) ->
KBCrop -> MultiScaleFlipAug(RandomFlip, Normalize) -> ``aug_test``; DDAD (``front_spec(cfg)['protocol'] == 'ddad'``):
LoadDDADImageFromFile(USEPE, USE_DYNAMIC_PE) -> DDADResize(shape, depth=False) -> MultiScaleFlipAug(flip=False, Normalize) ->
``simple_test``.  Per call, on the engine's stream (``FrameEngine._submit``):

  1. n uploads of uint8 BGR frames, each slot through its own pinned buffer (``PinnedUpload``), non-blocking;
  2. ONE front-end launch (csrc/infer.hip) writes the views of the n frames, frame-major and normalised, into the first ``views * n``
     images of the static ``(views * F, 5, H, W)`` input: ``ge_infer_front_batch`` (the frames may differ in size, as the KITTI days do;
     each has its own crop offsets and ground depth), ``ge_infer_front_ddad_batch`` (each frame its camera's ground depth; the n camera
     heights go through a pinned buffer into the static ``(F,)`` tensor the adaptive ground embedding reads through its device pointer,
     so a replayed graph follows them) or ``ge_infer_front_sweep`` (ONE frame under V <= F ground priors, include/gedepth_sweep.h).
     Outside the graph: only its arguments change from call to call;
  3. ``model.encode_decode`` runs all ``views * F`` images as one forward (clamped and rescaled, as ``inference`` does) and ONE
     ``ge_tta_merge_batch`` forms (view 0 + mirror(view 1)) / 2 per slot into the static ``(F, 1, H, W)`` output, in aug_test's order
     (a one-view config: a copy) — eagerly for ``WARMUP`` calls, then captured in a hipGraph and replayed.  KB crop and DDADResize make
     the forward's shape constant, so frames of every size share one graph;
  4. the first n maps go to the host, or stay in the static device buffer (``to_host=False``), valid until the next call.

A call of n < F frames fills the first n slots; the others keep what they held — zeros (the input is allocated with zeros), the smallest
known camera height, or an older frame — and the forward still runs on all F slots.  Only the n maps are ever returned: in eval mode no
operation of the model crosses samples (BatchNorm uses its running statistics, attention windows and the deformable attention stay
inside a sample), so what slot f holds does not reach another slot's map.

``_KITTIFront`` / ``_DDADFront`` hold what the protocols do differently: the argument errors of n frames and the filling of n slots.  The
engine has three faces: ``DepthInferencer`` (apis/inference.py; one slot, and the one-frame products ``ground_maps``, ``points``,
``scene_points``, ``error_map``), ``BatchDepthInferencer`` and ``BatchDDADInferencer`` (apis/batch_inference.py; ``batch``, ``run``,
``sweep``).  This module also holds the host helpers all of them use."""
import gc
import os.path as osp

import numpy as np
import torch
from PIL import Image

from ... import kernels as K
from ..datasets.pipelines import loading    # _DDAD_CAMERA_HEIGHT is read through the module at every use, so a changed table is seen
from ..utils.pinned import PinnedUpload

# test-time transforms of MultiScaleFlipAug the device front end restates (ImageToTensor / Collect are layout only)
_FRONT_TRANSFORMS = ('RandomFlip', 'Normalize', 'ImageToTensor', 'Collect')
_PROTOCOL = 'LoadImageFromFile(USEPE) -> KBCrop -> MultiScaleFlipAug(RandomFlip, Normalize)'
_DDAD_TRANSFORMS = ('Normalize', 'ImageToTensor', 'Collect')
_DDAD_PROTOCOL = ('LoadDDADImageFromFile(USEPE, USE_DYNAMIC_PE) -> DDADResize(shape, depth=False) -> '
                  'MultiScaleFlipAug(flip=False, Normalize)')


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


def _img_prefix(cfg):
    test = cfg.data.test
    img_dir, root = test.get('img_dir'), test.get('data_root')
    if img_dir is None:
        return root
    return img_dir if root is None or osp.isabs(img_dir) else osp.join(root, img_dir)


def _config_of(model):
    """``(front_spec, image prefix)`` of ``model.cfg``; host work only, so argument errors can be read off it before any device work."""
    cfg = getattr(model, 'cfg', None)
    if cfg is None:
        raise ValueError('model.cfg is missing: build the model with init_depther (or set model.cfg to its Config)')
    return front_spec(cfg), _img_prefix(cfg)


# ---- host helpers of the engines and the functions in front of them
def _decode(img):
    """A path (decoded as the host LoadImageFromFile does: PIL, RGB -> BGR) or an (H, W, 3) uint8 BGR array -> contiguous uint8 BGR."""
    if isinstance(img, str):
        return np.ascontiguousarray(np.asarray(Image.open(img).convert('RGB'))[..., ::-1])
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise TypeError(f'img must be a path or an (H, W, 3) uint8 BGR array, got {a.shape} {a.dtype}')
    return np.ascontiguousarray(a)


def frame_size(img):
    """(H, W) of a frame without decoding it: the PNG header of a path, the shape of an array."""
    if isinstance(img, str):
        with Image.open(img) as im:
            return im.size[1], im.size[0]
    return tuple(np.shape(img)[:2])


def _per_frame(value, n, error):
    """``value`` for each of ``n`` frames: a list holds one per frame (else ``ValueError(error)``), anything else serves every frame."""
    values = value if isinstance(value, list) else [value] * n
    if len(values) != n:
        raise ValueError(error.format(n=len(values), m=n))
    return values


def _paths_of(imgs):
    """The images that are paths, None for the arrays."""
    return [i if isinstance(i, str) else None for i in imgs]


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


def check_ground_source(spec, prefix, imgs, pes, calib):
    """``ValueError(_NO_PE)`` when a KITTI frame has no ground depth: no ``calib``, no ``pe`` of its own, no ``pe_165.npy`` in the test tree."""
    if calib is None and any(p is None and _pe_file(spec, prefix, i) is None for i, p in zip(imgs, pes)):
        raise ValueError(_NO_PE)


def check_kb_crop(spec, H, W):
    """``ValueError`` for a frame the KB crop does not fit into."""
    if H < spec['height'] or W < spec['width']:
        raise ValueError(f'frame {(H, W)} is smaller than the KB crop {(spec["height"], spec["width"])}')


def _check_count(n, slots, what='frames'):
    if not 1 <= n <= slots:
        raise ValueError(f'{n} {what} for an engine of {slots} slots')


# what a batch says of a frame without a camera; the one-slot engine has its own words (``FrameEngine.NO_CAMERA``)
_NO_CAMERA = 'no camera for frame {k}: pass cameras= (out of {known}) or image paths whose parent directory is the camera name'


def check_ddad_frames(spec, slots, sizes, pes, cameras, paths, frame_size=None, no_camera=_NO_CAMERA):
    """The argument errors of n DDAD frames, host work only -> ``(cameras, the frames' one (H, W))``.  ``sizes``: the frames' (H, W);
    ``pes`` / ``cameras`` / ``paths``: None or one entry per frame; ``frame_size``: what the engine has taken so far, or None."""
    n = len(sizes)
    _check_count(n, slots)
    for name, v in (('ground depths', pes), ('cameras', cameras), ('paths', paths)):
        if v is not None and len(v) != n:
            raise ValueError(f'{len(v)} {name} for {n} frames')
    cameras = cameras if cameras is not None else [None] * n
    paths = paths if paths is not None else [None] * n
    cams = [_ddad_camera(c, p) for c, p in zip(cameras, paths)]           # ValueError for a camera without a known height
    if any(c is None for c in cams):
        raise ValueError(no_camera.format(k=cams.index(None), known=', '.join(sorted(loading._DDAD_CAMERA_HEIGHT))))
    for H, W in sizes:
        if H < spec['height'] or W < spec['width']:
            raise ValueError(f'frame {(H, W)} is smaller than DDADResize\'s shape {(spec["height"], spec["width"])}')
        if frame_size is not None and frame_size != (H, W):
            raise ValueError(f'frame {(H, W)}: this engine takes frames of {frame_size} (reset() to change)')
        frame_size = (H, W)
    return cams, frame_size


# ---- the two protocols
class _KITTIFront:
    """KITTI's own part of n frames' way through a ``FrameEngine``; no state, the engine is handed in."""

    def check(self, eng, sizes, paths, cameras, pes):
        """The argument errors of n frames of ``sizes``, host work only -> ``(their cameras, the ori_shape of their metas)``; DDAD's also
        sets ``eng.frame_size``."""
        s = eng.spec
        _check_count(len(sizes), eng.frames)
        for H, W in sizes:
            check_kb_crop(s, H, W)
        return [None] * len(sizes), [(s['height'], s['width'], 5)] * len(sizes)

    def fill(self, eng, bgrs, paths, cams, pes, calib=None, cam_height=1.65, rows=None):
        """On the engine's stream, outside its graph: n ground depths, n uploads and ONE front-end launch into the first slots of
        ``static_in``; ``last_frames`` / ``last_ground_depths`` say what the slots were fed.  ``rows`` (the sweep): ONE frame, and the
        slots are its ``len(rows)`` variants."""
        s = eng.spec
        tops = [int(b.shape[0] - s['height']) for b in bgrs]                  # KBCrop
        lefts = [int((b.shape[1] - s['width']) / 2) for b in bgrs]
        raws = [eng.ground_depth(b.shape[0], b.shape[1], p, pe, calib, cam_height) for b, p, pe in zip(bgrs, paths, pes)]
        devs = [up(b, eng.device) for up, b in zip(eng._stagings, bgrs)]
        common = (s['mean'], s['std'], s['views'], s['to_rgb'], s['pe_max'], s['depth_scale'])
        if rows is None:
            K.infer_front_batch(devs, raws, eng.static_in, tops, lefts, *common)
        else:
            K.infer_front_sweep(devs[0], raws[0], rows, eng.static_in, tops[0], lefts[0], *common)
        copies = 1 if rows is None else len(rows)
        eng.last_ground_depths = raws * copies                # kept for ``scene_points`` and the stratified evaluation
        eng.last_frames = list(zip(devs, tops, lefts)) * copies        # kept for ``points`` and the error images


class _DDADFront:
    """DDAD's: the camera names ground depth and height, the frames of one engine have one size."""

    def check(self, eng, sizes, paths, cameras, pes):
        cams, eng.frame_size = check_ddad_frames(eng.spec, eng.frames, sizes, pes, cameras, paths, eng.frame_size, eng.NO_CAMERA)
        return cams, [(H, W, 5) for H, W in sizes]                     # LoadDDADImageFromFile: ori_shape = the frame's

    def fill(self, eng, bgrs, paths, cams, pes, calib=None, cam_height=None, rows=None):
        s = eng.spec
        raws = [eng.ground_depth_ddad(c, b.shape[0], b.shape[1], pe) for c, b, pe in zip(cams, bgrs, pes)]
        devs = [up(b, eng.device) for up, b in zip(eng._stagings, bgrs)]
        K.infer_front_ddad_batch(devs, raws, eng.static_in, s['mean'], s['std'], s['to_rgb'], s['pe_max'], s['depth_scale'])
        # one small copy into the tensor the captured forward reads through its device pointer; the order of PinnedUpload
        eng._heights[:len(cams)] = [float(loading._DDAD_CAMERA_HEIGHT[c]) for c in cams]       # the other slots keep the height they had
        if eng._heights_done is not None:
            eng._heights_done.synchronize()
        eng._heights_host.numpy()[...] = eng._heights
        eng.static_height.copy_(eng._heights_host, non_blocking=True)
        eng._heights_done = torch.cuda.Event()
        eng._heights_done.record()
        eng.last_cameras = cams


# ---- the engine
class FrameEngine:
    """The engine of one model, precision and count of frame slots (module docstring).  ``captures`` counts hipGraph captures and
    ``replays`` their replays; ``reset()`` drops the graphs and zeroes both.

    A capture is keyed by the precision and the ``kernel_variant`` of every module that has one.  It bakes in the addresses of the
    parameters, buffers and static tensors: parameters must be updated IN PLACE (``load_state_dict``, ``param.data.copy_``; ``FusedAdamW``
    updates its arena in place) for a replay to see them; replacing a parameter tensor needs ``reset()``.  Host-side heuristics evaluated
    at capture time (the cross-attention's query order) are frozen into the graph as in mmrt/graph.py; results do not depend on them.
    ``front``: the protocol's own part of a call."""

    WARMUP = 2
    NO_CAMERA = _NO_CAMERA

    def __init__(self, model, frames, bf16=False, config=None):
        self.model, self.frames, self.bf16 = model, frames, bool(bf16)
        self.spec, self.prefix = config or _config_of(model)
        self.ddad = self.spec['protocol'] == 'ddad'
        self.front = _DDADFront() if self.ddad else _KITTIFront()
        self.device = next(model.parameters()).device
        s, F = self.spec, frames
        # zeros, and a camera's height: a slot no frame has filled yet still holds finite values for the forward that runs over all slots
        self.static_in = torch.zeros(s['views'] * F, 5, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self._slots_out = torch.empty(F, 1, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self.static_out = self._public_out(self._slots_out)
        self.static_height, self._forward_kw = None, {}
        if self.ddad:                 # the camera heights, filled per call outside the graph; ground_embed_adaptive reads them through the device pointer
            self._heights = [float(min(loading._DDAD_CAMERA_HEIGHT.values()))] * F
            self.static_height = torch.tensor(self._heights, device=self.device, dtype=torch.float32)
            self._forward_kw = dict(height=self.static_height)           # no ``test`` key: _height takes the tensor as it is
            self._heights_host, self._heights_done = torch.empty(F, dtype=torch.float32, pin_memory=True), None
        self.stream = torch.cuda.Stream(self.device)
        self._stagings = [PinnedUpload() for _ in range(F)]
        self._pe = {}
        self.reset()

    def _public_out(self, slots):
        """What ``static_out`` is of the ``(F, 1, H, W)`` output: all of it; the one-slot engine shows its one ``(1, H, W)`` map."""
        return slots

    def reset(self):
        """Drop every captured graph (and its memory pool) and the warm-up counts."""
        self.graphs, self.calls, self.captures, self.replays = {}, {}, 0, 0
        self.frame_size = None                       # DDAD: the (H, W) of the frames this engine has taken
        self.last_n = 0                              # the frame count of the last call
        self.last_ground_depths = None               # KITTI: the raw (H, W) f32 ground depths the last call's front end was given
        self.last_frames = None                      # KITTI: [(device uint8 BGR frame, top, left)] of the last call
        self.last_cameras = None                     # DDAD: the cameras of the last call

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

    # ---- one call
    def _key(self, ground=False):
        key = (self.bf16,) + tuple(m.kernel_variant for m in self.model.modules() if hasattr(m, 'kernel_variant'))
        return key + ('ground',) if ground else key

    def _metas(self, paths, sizes, ori_shapes):
        """The ``views`` metas of each frame, frame-major."""
        s = self.spec
        norm = dict(mean=np.float32(s['mean']), std=np.float32(s['std']), to_rgb=s['to_rgb'])
        return [dict(filename=p, ori_filename=p, ori_shape=ori, img_shape=tuple(shape) + (5,), pad_shape=tuple(shape) + (5,),
                     scale_factor=1.0, flip=bool(v), flip_direction='horizontal', img_norm_cfg=norm)
                for p, shape, ori in zip(paths, sizes, ori_shapes) for v in range(s['views'])]

    def _body(self, metas, ground=False):
        """The forward over all F slots and their merge; ``ground`` (one slot): ``ge_ground_maps`` behind it, for ``ground_maps``."""
        model = self.model
        model.keep_ground_lr = ground                # the forward keeps the two ground necks' low-resolution outputs for ge_ground_maps
        try:
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.bf16):
                pred = model.encode_decode(self.static_in, metas, rescale=True, **self._forward_kw)
            lr, model.ground_lr = model.ground_lr, None
        finally:
            model.keep_ground_lr = False
        if self.spec['views'] == 2:
            K.tta_merge_batch(pred.float().contiguous(), self._slots_out)       # all F slots: the captured launch does not depend on n
        else:
            self._slots_out.copy_(pred)
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

    def _submit(self, n, fill, metas, graph, tail, ground=False):
        """Every forward of the engine: the caller's current stream -> the engine's; ``fill()``, the per-call work outside the graph,
        into the first ``n`` slots; ``_run`` of the body over all F slots (``metas``: those of the n frames; the other slots repeat the
        last frame's); ``tail()`` -> what the call returns (a host copy, which synchronises the engine's stream, or views of the static
        buffers); then back: the caller's stream waits for the engine's."""
        metas = metas + metas[-self.spec['views']:] * (self.frames - n)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            fill()
            self._run(self._key(ground), graph, lambda: self._body(metas, ground))
            self.last_n = n
            out = tail()
        cur.wait_stream(self.stream)
        return out

    def _after(self, work):
        """``work()`` on the engine's stream behind the last call's frame (a kernel that reads its map); the caller's stream waits for it."""
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            out = work()
        cur.wait_stream(self.stream)
        return out
