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
inflating) while the device computes the current one.  DDAD, ``points`` and ``ground_maps`` stay single-frame (``DepthInferencer``)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from ... import kernels as K
from ...batch_kernels import BATCH_MAX
from ..utils.pinned import PinnedUpload
from .inference import DepthInferencer, _config_of, _decode

__all__ = ['BatchDepthInferencer', 'check_batch', 'decode_ahead', 'DECODE_WORKERS']

DECODE_WORKERS = 4                 # a constant, never the machine's core count: decoding one batch ahead needs no more


def check_batch(batch, spec=None, what='batch'):
    """The argument errors of a frame count, before any device work: 1 .. 8, and more than 1 on the KITTI protocol only."""
    if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= BATCH_MAX:
        raise ValueError(f'{what} must be an integer in 1 .. {BATCH_MAX} (the frame slots of one ge_infer_front_batch launch), got {batch!r}')
    if batch > 1 and spec is not None and spec['protocol'] == 'ddad':
        raise NotImplementedError(f'{what}={batch} with a DDAD config: the batched engine implements the KITTI protocol only; DDAD frames '
                                  f'run one at a time ({what}=1)')
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


class BatchDepthInferencer(DepthInferencer):
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

    def _key(self, ground=False):
        return super()._key(ground) + ('batch', self.frames)

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
        n, s = len(imgs), self.spec
        if not 1 <= n <= self.frames:
            raise ValueError(f'{n} frames for an engine of {self.frames} slots')
        pes = pes if pes is not None else [None] * n
        paths = paths if paths is not None else [i if isinstance(i, str) else None for i in imgs]
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
            self.last_n = n
            if to_host:
                host = self.static_out[:n].cpu().numpy()                           # synchronises the engine's stream
                out = [host[f].copy() for f in range(n)]
            else:
                out = self.static_out[:n]
        cur.wait_stream(self.stream)
        return out

    def reset(self):
        super().reset()
        self.last_n = 0                              # the frame count of the last batch
        self.last_ground_depths = None               # the raw (H, W) f32 ground depths the last batch's front end was given
        self.last_frames = None                      # [(device uint8 BGR frame, top, left)] of the last batch, for the error images

    def run(self, imgs, pes=None, calib=None, cam_height=1.65, graph=True):
        """Any number of frames, in batches of F with the next batch decoding ahead -> one host map per frame, in order."""
        pes = pes if pes is not None else [None] * len(imgs)
        F, out = self.frames, []
        for k, bgrs in enumerate(decode_ahead([(lambda i=i: _decode(i)) for i in imgs], F)):
            part = slice(k * F, k * F + len(bgrs))
            out += self.batch(bgrs, pes[part], calib, cam_height, graph, paths=[i if isinstance(i, str) else None for i in imgs[part]])
        return out
