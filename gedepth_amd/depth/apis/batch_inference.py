"""Depth for several KITTI frames per forward: ``BatchDepthInferencer``, the engine of apis/inference.py with F <= 8 frame slots.

Per batch of n <= F frames, on the engine's stream:

  1. n uploads, each slot through its own pinned buffer (``PinnedUpload``), non-blocking;
  2. ONE ``ge_infer_front_batch`` (csrc/infer.hip) writes the flip views of the n frames, frame-major, into the first ``views * n``
     images of the static ``(views * F, 5, 352, 1216)`` input; the frames may differ in size (the KITTI days do), each has its own crop
     offsets and ground depth.  Outside the graph: only its arguments change from batch to batch;
  3. ``model.encode_decode`` runs all ``views * F`` images as one forward and ONE ``ge_tta_merge_batch`` merges the F pairs into the
     static ``(F, 1, 352, 1216)`` output (a one-view config: a copy) — captured in a hipGraph after ``WARMUP`` eager batches;
  4. the first n maps go to the host, or stay on the device (``to_host=False``).

A last batch of n < F frames fills the first n slots; the others keep what they held — zeros (the input is allocated with zeros) or an
older frame — and the forward still runs on all F slots.  Only the n maps are ever returned: in eval mode no operation of the model
crosses samples (BatchNorm uses its running statistics, attention windows and the deformable attention stay inside a sample), so what
slot f holds does not reach another slot's map.

``decode_ahead`` is the host side: a pool of at most ``DECODE_WORKERS`` threads decodes the next batch's PNGs (PIL releases the GIL while
inflating) while the device computes the current one.  ``points`` and ``ground_maps`` stay single-frame (``DepthInferencer``).

``BatchDepthInferencer.sweep`` fills the slots with ONE frame under V <= F ground priors instead (include/gedepth_sweep.h: a global pitch,
a height scale, the prior removed): one upload and one ``ge_infer_front_sweep`` launch in place of step 1 and 2, then steps 3 and 4
unchanged, on the same captured graph.

``BatchDDADInferencer`` is the same engine for the DDAD protocol (one view per frame, no merge): n uploads, ONE
``ge_infer_front_ddad_batch`` into the first n images of the static ``(F, 5, Hd, Wd)`` input, the n cameras' heights into the static
``(F,)`` tensor the adaptive ground embedding reads (one small copy, outside the graph), one captured forward over all F slots.  The slots
of a batch may hold different cameras.  ``inference_depther(batch > 1)`` stays refused for a DDAD config (``check_batch``): files to
maps in batches is ``BatchDDADInferencer.run``, the loop's route is ``single_gpu_test(device_eval=True, eval_batch=F)``."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from ... import kernels as K
from ...batch_kernels import BATCH_MAX
from ..utils.pinned import PinnedUpload
from ..datasets.pipelines import loading    # _DDAD_CAMERA_HEIGHT is read through the module at every use, as apis/inference.py does
from .inference import DepthInferencer, _config_of, _ddad_camera, _decode, _per_frame

__all__ = ['BatchDepthInferencer', 'BatchDDADInferencer', 'check_batch', 'check_ddad_batch', 'decode_ahead', 'DECODE_WORKERS']

DECODE_WORKERS = 4                 # a constant, never the machine's core count: decoding one batch ahead needs no more


def check_batch(batch, spec=None, what='batch', ddad=False):
    """The argument errors of a frame count, before any device work: 1 .. 8, and more than 1 on the KITTI protocol only — unless the
    caller has a DDAD route (``ddad=True``: the device evaluation loop, which runs a ``BatchDDADInferencer``; ``inference_depther`` has
    none and keeps refusing)."""
    if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= BATCH_MAX:
        raise ValueError(f'{what} must be an integer in 1 .. {BATCH_MAX} (the frame slots of one ge_infer_front_batch launch), got {batch!r}')
    if batch > 1 and not ddad and spec is not None and spec['protocol'] == 'ddad':
        raise NotImplementedError(f'{what}={batch} with a DDAD config: the batched engine implements the KITTI protocol only; DDAD frames '
                                  f'run one at a time ({what}=1), or in batches through BatchDDADInferencer.run and '
                                  'single_gpu_test(device_eval=True, eval_batch=F)')
    return batch


def decode_ahead(jobs, size, workers=DECODE_WORKERS):
    """``jobs``: one zero-argument callable per frame (its host-side decoding).  Yields their results in lists of ``size`` (the last one
    shorter), in order, with the NEXT list's jobs already running on a pool of ``min(workers, DECODE_WORKERS, size)`` threads while the
    caller works on the current one.  An exception of a job is raised when its list is due."""
    chunks = [jobs[i:i + size] for i in range(0, len(jobs), size)]
    if not chunks:
        return
    with ThreadPoolExecutor(max_workers=max(1, min(workers, DECODE_WORKERS, size))) as pool:
        ahead = [pool.submit(j) for j in chunks[0]]
        for k in range(len(chunks)):
            current = ahead
            ahead = [pool.submit(j) for j in chunks[k + 1]] if k + 1 < len(chunks) else []
            try:
                yield [f.result() for f in current]
            except BaseException:
                for f in ahead:
                    f.cancel()
                raise


def frame_size(img):
    """(H, W) of a frame without decoding it: the PNG header of a path, the shape of an array."""
    if isinstance(img, str):
        with Image.open(img) as im:
            return im.size[1], im.size[0]
    return tuple(np.shape(img)[:2])


class _BatchEngine(DepthInferencer):
    """What the two engines of ``frames`` = F slots share: the capture key, the head and the tail of ``batch``, the chunks of ``run``
    and what ``reset`` clears.  The front-end calls, the forward and the order of work on the engine's stream are each engine's own."""

    # plain attributes (the base class derives them from its one frame): a batch keeps lists of its own under these names
    last_frames = last_ground_depths = None

    def _key(self, ground=False):
        return super()._key(ground) + ('batch', self.frames)

    def _head(self, imgs, paths):
        """The frame count of ``batch(imgs)`` against the slots -> ``(n, paths, by default the images that are paths)``."""
        n = len(imgs)
        if not 1 <= n <= self.frames:
            raise ValueError(f'{n} frames for an engine of {self.frames} slots')
        return n, paths if paths is not None else [i if isinstance(i, str) else None for i in imgs]

    def _maps(self, n, to_host):
        """The tail of ``batch``, on the engine's stream behind ``_run``: n fresh host arrays, or the view ``static_out[:n]``."""
        self.last_n = n
        if not to_host:
            return self.static_out[:n]
        host = self.static_out[:n].cpu().numpy()                               # synchronises the engine's stream
        return [host[f].copy() for f in range(n)]

    def _chunks(self, imgs):
        """``run``'s frames in batches of F, the next batch decoding ahead -> ``(their slice of imgs, the decoded frames)``."""
        for k, bgrs in enumerate(decode_ahead([(lambda i=i: _decode(i)) for i in imgs], self.frames)):
            yield slice(k * self.frames, k * self.frames + len(bgrs)), bgrs

    def reset(self):
        super().reset()
        self.last_n = 0                              # the frame count of the last batch
        self.last_ground_depths = None               # KITTI: the raw (H, W) f32 ground depths the last batch's front end was given
        self.last_frames = None                      # KITTI: [(device uint8 BGR frame, top, left)] of the last batch, for the error images


class BatchDepthInferencer(_BatchEngine):
    """The flip-TTA engine with ``frames`` = F slots (module docstring); KITTI protocol.  ``batch(imgs)`` runs n <= F frames.  Captures are
    keyed as ``DepthInferencer``'s plus ``('batch', F)``; the capture itself (``_run``) and the contract that parameters are updated IN PLACE
    (a replay then sees the new values: ``FusedAdamW`` updates its arena in place) are the base class's."""

    def __init__(self, model, frames, bf16=False, config=None):
        config = config or _config_of(model)
        self.frames = check_batch(frames, config[0], 'frames')
        super().__init__(model, bf16, config)
        if self.ddad:
            raise NotImplementedError('BatchDepthInferencer with a DDAD config: the batched engine implements the KITTI protocol only')
        s, F = self.spec, self.frames
        # zeros: a slot no frame has filled yet still holds finite values for the forward that runs over all slots
        self.static_in = torch.zeros(s['views'] * F, 5, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self.static_out = torch.empty(F, 1, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self._stagings = [PinnedUpload() for _ in range(F)]

    def _body(self, metas, ground=False):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.bf16):
            pred = self.model.encode_decode(self.static_in, metas, rescale=True)
        pred = pred.float().contiguous()
        if self.spec['views'] == 2:
            K.tta_merge_batch(pred, self.static_out)          # all F slots: the captured launch does not depend on n
        else:
            self.static_out.copy_(pred)

    def _single(self, *a, **kw):
        raise NotImplementedError('a BatchDepthInferencer runs batch(imgs); single frames, points, scene_points, error_map and ground_maps go through the '
                                  'DepthInferencer of engine_for(model, bf16)')

    __call__ = ground_maps = points = scene_points = error_map = _single

    def batch(self, imgs, pes=None, calib=None, cam_height=1.65, graph=True, to_host=True, paths=None):
        """n <= F frames -> their maps.  ``imgs``: paths, (H, W, 3) uint8 BGR arrays, or frames already decoded by ``decode_ahead`` (then
        ``paths`` names their files, for the ground depth of the test tree); ``pes``: one raw ground depth per frame or None.  Returns a
        list of n fresh (1, 352, 1216) float32 host arrays, or with ``to_host=False`` the view ``static_out[:n]`` of the static device
        buffer, without synchronising: valid until the next call, ordered on ``self.stream``."""
        (n, paths), s = self._head(imgs, paths), self.spec
        pes = pes if pes is not None else [None] * n
        bgrs = [_decode(i) for i in imgs]
        for b in bgrs:
            self.front.frame(self, b.shape[0], b.shape[1], None, None)           # a frame smaller than the crop, before any device work
        metas = [m for b, p in zip(bgrs, paths) for m in self._metas(p, b.shape[:2], (s['height'], s['width'], 5))]
        metas += metas[-s['views']:] * (self.frames - n)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            tops = [int(b.shape[0] - s['height']) for b in bgrs]                  # KBCrop
            lefts = [int((b.shape[1] - s['width']) / 2) for b in bgrs]
            raws = [self.ground_depth(b.shape[0], b.shape[1], p, pe, calib, cam_height) for b, p, pe in zip(bgrs, paths, pes)]
            self.last_ground_depths = raws                    # kept for the stratified evaluation, as last_ground_depth is
            devs = [up(b, self.device) for up, b in zip(self._stagings, bgrs)]
            K.infer_front_batch(devs, raws, self.static_in, tops, lefts, s['mean'], s['std'], s['views'], s['to_rgb'], s['pe_max'],
                                s['depth_scale'])
            self.last_frames = list(zip(devs, tops, lefts))   # kept for the error images, as last_frame is
            self._run(self._key(), graph, lambda: self._body(metas))
            out = self._maps(n, to_host)
        cur.wait_stream(self.stream)
        return out

    def sweep(self, img, variants, pe=None, calib=None, cam_height=1.65, graph=True, to_host=True, path=None):
        """ONE frame under V = ``len(variants)`` <= F ground priors -> its V maps, in the variants' order.  ``variants``: a
        ``core.PriorSweep`` or its ``(c, s, drop)`` rows (include/gedepth_sweep.h states the rule); ``img``, ``pe``, ``calib``,
        ``cam_height``, ``path`` as one frame of ``batch``.  One decode, one upload (slot 0's pinned buffer), one ``ground_depth`` and ONE
        ``ge_infer_front_sweep`` launch fill the first ``views * V`` images of ``static_in``; the forward is ``batch``'s, under its
        key and on its static buffers, so both share one captured graph.  Slots from V on keep what they held.  Returns as ``batch``;
        ``last_ground_depths`` / ``last_frames`` hold the unperturbed plane / the uploaded frame V times."""
        from ...sweep_kernels import variant_table
        rows = variants.table() if hasattr(variants, 'table') else list(variants)
        V, s = len(variant_table(rows)), self.spec                              # the rows' argument errors, before any device work
        if V > self.frames:
            raise ValueError(f'{V} variants for an engine of {self.frames} slots')
        path = path if path is not None else (img if isinstance(img, str) else None)
        bgr = _decode(img)
        H, W = bgr.shape[:2]
        self.front.frame(self, H, W, None, None)                                  # a frame smaller than the crop, before any device work
        metas = self._metas(path, (H, W), (s['height'], s['width'], 5)) * self.frames
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            top, left = int(H - s['height']), int((W - s['width']) / 2)          # KBCrop
            raw = self.ground_depth(H, W, path, pe, calib, cam_height)
            dev = self._stagings[0](bgr, self.device)
            K.infer_front_sweep(dev, raw, rows, self.static_in, top, left, s['mean'], s['std'], s['views'], s['to_rgb'], s['pe_max'],
                                s['depth_scale'])
            self.last_ground_depths, self.last_frames = [raw] * V, [(dev, top, left)] * V
            self._run(self._key(), graph, lambda: self._body(metas))
            out = self._maps(V, to_host)
        cur.wait_stream(self.stream)
        return out

    def run(self, imgs, pes=None, calib=None, cam_height=1.65, graph=True):
        """Any number of frames, in batches of F with the next batch decoding ahead -> one host map per frame, in order."""
        pes = pes if pes is not None else [None] * len(imgs)
        out = []
        for part, bgrs in self._chunks(imgs):
            out += self.batch(bgrs, pes[part], calib, cam_height, graph, paths=[i if isinstance(i, str) else None for i in imgs[part]])
        return out


def check_ddad_batch(spec, slots, sizes, pes, cameras, paths, frame_size=None):
    """The argument errors of one DDAD batch, host work only -> ``(cameras, the frames' one (H, W))``.  ``sizes``: the frames' (H, W);
    ``pes`` / ``cameras`` / ``paths``: None or one entry per frame; ``frame_size``: what the engine has taken so far, or None."""
    n = len(sizes)
    if not 1 <= n <= slots:
        raise ValueError(f'{n} frames for an engine of {slots} slots')
    for name, v in (('ground depths', pes), ('cameras', cameras), ('paths', paths)):
        if v is not None and len(v) != n:
            raise ValueError(f'{len(v)} {name} for {n} frames')
    cameras = cameras if cameras is not None else [None] * n
    paths = paths if paths is not None else [None] * n
    cams = [_ddad_camera(c, p) for c, p in zip(cameras, paths)]           # ValueError for a camera without a known height
    if any(c is None for c in cams):
        raise ValueError(f'no camera for frame {cams.index(None)}: pass cameras= (out of {", ".join(sorted(loading._DDAD_CAMERA_HEIGHT))}) or '
                         'image paths whose parent directory is the camera name')
    for H, W in sizes:
        if H < spec['height'] or W < spec['width']:
            raise ValueError(f'frame {(H, W)} is smaller than DDADResize\'s shape {(spec["height"], spec["width"])}')
        if frame_size is not None and frame_size != (H, W):
            raise ValueError(f'frame {(H, W)}: this engine takes frames of {frame_size} (reset() to change)')
        frame_size = (H, W)
    return cams, frame_size


class BatchDDADInferencer(_BatchEngine):
    """The DDAD engine with ``frames`` = F slots (module docstring).  ``batch(imgs)`` runs n <= F frames, which may come from different
    cameras: each slot has its own ground depth and its own entry of ``static_height``.  Captures are keyed as ``DepthInferencer``'s plus
    ``('batch', F)``; the capture itself and the in-place contract on the parameters are the base class's, and so is the rule that one
    engine takes frames of one size."""

    def __init__(self, model, frames, bf16=False, config=None):
        config = config or _config_of(model)
        self.frames = check_batch(frames, what='frames')
        if config[0]['protocol'] != 'ddad':
            raise NotImplementedError('BatchDDADInferencer with a KITTI config: the KITTI protocol runs in a BatchDepthInferencer')
        super().__init__(model, bf16, config)
        s, F = self.spec, self.frames
        # zeros, and a camera's height: a slot no frame has filled yet still holds finite values for the forward that runs over all slots
        self.static_in = torch.zeros(F, 5, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self.static_out = torch.empty(F, 1, s['height'], s['width'], device=self.device, dtype=torch.float32)
        self._heights = [float(min(loading._DDAD_CAMERA_HEIGHT.values()))] * F
        self.static_height = torch.tensor(self._heights, device=self.device, dtype=torch.float32)
        self._forward_kw = dict(height=self.static_height)
        self._heights_host, self._heights_done = torch.empty(F, dtype=torch.float32, pin_memory=True), None
        self._stagings = [PinnedUpload() for _ in range(F)]

    def _body(self, metas, ground=False):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.bf16):
            pred = self.model.encode_decode(self.static_in, metas, rescale=True, **self._forward_kw)
        self.static_out.copy_(pred)                           # all F slots: the captured forward does not depend on n

    def _single(self, *a, **kw):
        raise NotImplementedError('a BatchDDADInferencer runs batch(imgs); single frames and ground_maps go through the DepthInferencer of '
                                  'engine_for(model, bf16); points, scene_points and error_map are built for the KITTI protocol')

    __call__ = ground_maps = points = scene_points = error_map = _single

    def batch(self, imgs, pes=None, cameras=None, graph=True, to_host=True, paths=None):
        """n <= F frames -> their maps.  ``imgs``: paths, (H, W, 3) uint8 BGR arrays, or frames already decoded by ``decode_ahead`` (then
        ``paths`` names their files, for the camera); ``pes``: one raw ground depth per frame (an entry may be None) or None: the
        camera's ``ddad_pe.npz``; ``cameras``: one name per frame (an entry may be None) or None: the path's parent directory.  Returns a
        list of n fresh (1, Hd, Wd) float32 host arrays, or with ``to_host=False`` the view ``static_out[:n]`` of the static device
        buffer, without synchronising: valid until the next call, ordered on ``self.stream``.  Every argument error is raised before any
        device work."""
        (n, paths), s = self._head(imgs, paths), self.spec
        if len(paths) != n:
            raise ValueError(f'{len(paths)} paths for {n} frames')
        bgrs = [_decode(i) for i in imgs]
        cams, self.frame_size = check_ddad_batch(s, self.frames, [b.shape[:2] for b in bgrs], pes, cameras, paths, self.frame_size)
        pes = pes if pes is not None else [None] * n
        metas = [m for b, p in zip(bgrs, paths) for m in self._metas(p, b.shape[:2], tuple(b.shape[:2]) + (5,))]
        metas += metas[-1:] * (self.frames - n)
        self._heights[:n] = [float(loading._DDAD_CAMERA_HEIGHT[c]) for c in cams]      # the other slots keep the height they had
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            raws = [self.ground_depth_ddad(c, b.shape[0], b.shape[1], pe) for c, b, pe in zip(cams, bgrs, pes)]
            devs = [up(b, self.device) for up, b in zip(self._stagings, bgrs)]
            K.infer_front_ddad_batch(devs, raws, self.static_in, s['mean'], s['std'], s['to_rgb'], s['pe_max'], s['depth_scale'])
            # one small copy into the tensor the captured forward reads through its device pointer; the order of PinnedUpload
            if self._heights_done is not None:
                self._heights_done.synchronize()
            self._heights_host.numpy()[...] = self._heights
            self.static_height.copy_(self._heights_host, non_blocking=True)
            self._heights_done = torch.cuda.Event()
            self._heights_done.record()
            self._run(self._key(), graph, lambda: self._body(metas))
            self.last_cameras = cams
            out = self._maps(n, to_host)
        cur.wait_stream(self.stream)
        return out

    def reset(self):
        super().reset()
        self.last_cameras = None                     # the cameras of the last batch

    def run(self, imgs, pes=None, cameras=None, graph=True):
        """Any number of frames, in batches of F with the next batch decoding ahead -> one host map per frame, in order: the files-to-maps
        route of a DDAD config (``inference_depther(batch > 1)`` refuses it).  ``pes`` / ``cameras``: a value for every frame, or a
        list with one per frame."""
        imgs = imgs if isinstance(imgs, list) else [imgs]
        pes = _per_frame(pes, len(imgs), '{n} ground-depth maps for {m} frames')
        cameras = _per_frame(cameras, len(imgs), '{n} cameras for {m} frames')
        paths = [i if isinstance(i, str) else None for i in imgs]
        for c, p in zip(cameras, paths):                                          # every frame's camera, before the first batch runs
            if _ddad_camera(c, p) is None:
                raise ValueError(f'no camera for a frame: pass cameras= (out of {", ".join(sorted(loading._DDAD_CAMERA_HEIGHT))}) or image '
                                 'paths whose parent directory is the camera name')
        out = []
        for part, bgrs in self._chunks(imgs):
            out += self.batch(bgrs, pes[part], cameras[part], graph, paths=paths[part])
        return out
