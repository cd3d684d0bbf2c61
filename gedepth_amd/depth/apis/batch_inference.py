"""Depth for several frames per forward: the F-slot faces of the frame engine (apis/engine.py has the engine and its steps).

``BatchDepthInferencer`` (KITTI protocol): ``batch(imgs)`` runs n <= F frames, which may differ in size; ``sweep`` fills the slots with
ONE frame under V <= F ground priors instead (include/gedepth_sweep.h: a global pitch, a height scale, the prior removed), on the same
captured graph.  ``BatchDDADInferencer`` (DDAD protocol; one view per frame, no merge): the slots of a batch may hold different cameras,
each with its own ground depth and its own entry of ``static_height``.  ``run`` of either takes any number of frames in batches of F.
``inference_depther(batch > 1)`` stays refused for a DDAD config (``check_batch``): files to maps in batches is
``BatchDDADInferencer.run``, the loop's route is ``single_gpu_test(device_eval=True, eval_batch=F)``.  ``ground_maps``, ``points``,
``scene_points`` and ``error_map`` stay single-frame (``DepthInferencer``).

``decode_ahead`` is the host side: a pool of at most ``DECODE_WORKERS`` threads decodes the next batch's PNGs (PIL releases the GIL while
inflating) while the device computes the current one."""
from concurrent.futures import ThreadPoolExecutor

from ...batch_kernels import BATCH_MAX
from ...sweep_kernels import variant_table
from ..datasets.pipelines import loading    # _DDAD_CAMERA_HEIGHT is read through the module at every use, as apis/engine.py does
from .engine import FrameEngine, _check_count, _config_of, _ddad_camera, _decode, _paths_of, _per_frame, check_ddad_frames

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


def check_ddad_batch(spec, slots, sizes, pes, cameras, paths, frame_size=None):
    """The argument errors of one DDAD batch, host work only -> ``(cameras, the frames' one (H, W))``: the DDAD front's own check
    (``engine.check_ddad_frames``) in a batch's words."""
    return check_ddad_frames(spec, slots, sizes, pes, cameras, paths, frame_size)


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


class _BatchEngine(FrameEngine):
    """What the two faces with ``frames`` = F slots share: the capture key, ``batch`` behind its argument lists, its tail and the chunks
    of ``run``."""

    def _key(self, ground=False):
        return super()._key(ground) + ('batch', self.frames)

    def _batch(self, imgs, paths, pes, cameras, graph, to_host, **own):
        """n <= F frames through the front's check (every argument error before any device work) and ``_submit``."""
        paths = paths if paths is not None else _paths_of(imgs)
        bgrs = [_decode(i) for i in imgs]
        n, sizes = len(bgrs), [b.shape[:2] for b in bgrs]
        cams, oris = self.front.check(self, sizes, paths, cameras, pes)
        pes = pes if pes is not None else [None] * n
        return self._submit(n, lambda: self.front.fill(self, bgrs, paths, cams, pes, **own), self._metas(paths, sizes, oris), graph,
                            lambda: self._maps(n, to_host))

    def _maps(self, n, to_host):
        """The tail of a call, on the engine's stream behind ``_run``: n fresh host arrays, or the view ``static_out[:n]``."""
        if not to_host:
            return self.static_out[:n]
        host = self.static_out[:n].cpu().numpy()                               # synchronises the engine's stream
        return [host[f].copy() for f in range(n)]

    def _chunks(self, imgs):
        """``run``'s frames in batches of F, the next batch decoding ahead -> ``(their slice of imgs, the decoded frames)``."""
        for k, bgrs in enumerate(decode_ahead([(lambda i=i: _decode(i)) for i in imgs], self.frames)):
            yield slice(k * self.frames, k * self.frames + len(bgrs)), bgrs


class BatchDepthInferencer(_BatchEngine):
    """The flip-TTA engine with ``frames`` = F slots; KITTI protocol.  ``batch(imgs)`` runs n <= F frames, ``sweep`` one frame under V <= F
    ground priors.  Captures are keyed as ``DepthInferencer``'s plus ``('batch', F)``."""

    def __init__(self, model, frames, bf16=False, config=None):
        config = config or _config_of(model)
        check_batch(frames, config[0], 'frames')
        if config[0]['protocol'] == 'ddad':
            raise NotImplementedError('BatchDepthInferencer with a DDAD config: the batched engine implements the KITTI protocol only')
        super().__init__(model, frames, bf16, config)

    def _single(self, *a, **kw):
        raise NotImplementedError('a BatchDepthInferencer runs batch(imgs); single frames, points, scene_points, error_map and ground_maps go through the '
                                  'DepthInferencer of engine_for(model, bf16)')

    __call__ = ground_maps = points = scene_points = error_map = _single

    def batch(self, imgs, pes=None, calib=None, cam_height=1.65, graph=True, to_host=True, paths=None):
        """n <= F frames -> their maps.  ``imgs``: paths, (H, W, 3) uint8 BGR arrays, or frames already decoded by ``decode_ahead`` (then
        ``paths`` names their files, for the ground depth of the test tree); ``pes``: one raw ground depth per frame or None.  Returns a
        list of n fresh (1, 352, 1216) float32 host arrays, or with ``to_host=False`` the view ``static_out[:n]`` of the static device
        buffer, without synchronising: valid until the next call, ordered on ``self.stream``."""
        return self._batch(imgs, paths, pes, None, graph, to_host, calib=calib, cam_height=cam_height)

    def sweep(self, img, variants, pe=None, calib=None, cam_height=1.65, graph=True, to_host=True, path=None):
        """ONE frame under V = ``len(variants)`` <= F ground priors -> its V maps, in the variants' order.  ``variants``: a
        ``core.PriorSweep`` or its ``(c, s, drop)`` rows (include/gedepth_sweep.h states the rule); ``img``, ``pe``, ``calib``,
        ``cam_height``, ``path`` as one frame of ``batch``.  One decode, one upload (slot 0's pinned buffer), one ``ground_depth`` and ONE
        ``ge_infer_front_sweep`` launch fill the first ``views * V`` images of ``static_in``; the forward is ``batch``'s, under its
        key and on its static buffers, so both share one captured graph.  Slots from V on keep what they held.  Returns as ``batch``;
        ``last_ground_depths`` / ``last_frames`` hold the unperturbed plane / the uploaded frame V times."""
        rows = variants.table() if hasattr(variants, 'table') else list(variants)
        V = len(variant_table(rows))                                            # the rows' argument errors, before any device work
        _check_count(V, self.frames, 'variants')
        paths = [path if path is not None else (img if isinstance(img, str) else None)]
        bgr = _decode(img)
        sizes = [bgr.shape[:2]]
        _, oris = self.front.check(self, sizes, paths, None, None)                # a frame smaller than the crop, before any device work
        return self._submit(V, lambda: self.front.fill(self, [bgr], paths, None, [pe], calib, cam_height, rows),
                            self._metas(paths, sizes, oris) * V, graph, lambda: self._maps(V, to_host))

    def run(self, imgs, pes=None, calib=None, cam_height=1.65, graph=True):
        """Any number of frames, in batches of F with the next batch decoding ahead -> one host map per frame, in order."""
        pes = pes if pes is not None else [None] * len(imgs)
        out = []
        for part, bgrs in self._chunks(imgs):
            out += self.batch(bgrs, pes[part], calib, cam_height, graph, paths=_paths_of(imgs[part]))
        return out


class BatchDDADInferencer(_BatchEngine):
    """The DDAD engine with ``frames`` = F slots.  ``batch(imgs)`` runs n <= F frames, which may come from different cameras.  Captures
    are keyed as ``DepthInferencer``'s plus ``('batch', F)``; one engine takes frames of one size."""

    def __init__(self, model, frames, bf16=False, config=None):
        config = config or _config_of(model)
        check_batch(frames, what='frames')
        if config[0]['protocol'] != 'ddad':
            raise NotImplementedError('BatchDDADInferencer with a KITTI config: the KITTI protocol runs in a BatchDepthInferencer')
        super().__init__(model, frames, bf16, config)

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
        return self._batch(imgs, paths, pes, cameras, graph, to_host)

    def run(self, imgs, pes=None, cameras=None, graph=True):
        """Any number of frames, in batches of F with the next batch decoding ahead -> one host map per frame, in order: the files-to-maps
        route of a DDAD config (``inference_depther(batch > 1)`` refuses it).  ``pes`` / ``cameras``: a value for every frame, or a
        list with one per frame."""
        imgs = imgs if isinstance(imgs, list) else [imgs]
        pes = _per_frame(pes, len(imgs), '{n} ground-depth maps for {m} frames')
        cameras = _per_frame(cameras, len(imgs), '{n} cameras for {m} frames')
        paths = _paths_of(imgs)
        for c, p in zip(cameras, paths):                                          # every frame's camera, before the first batch runs
            if _ddad_camera(c, p) is None:
                raise ValueError(f'no camera for a frame: pass cameras= (out of {", ".join(sorted(loading._DDAD_CAMERA_HEIGHT))}) or image '
                                 'paths whose parent directory is the camera name')
        out = []
        for part, bgrs in self._chunks(imgs):
            out += self.batch(bgrs, pes[part], cameras[part], graph, paths=paths[part])
        return out
