"""Evaluation loops (depth/apis/test.py:32-232): run the model with ``return_loss=False`` over a data loader and either
keep the predictions or reduce them to per-image metric tuples on the fly (``pre_eval``).  With ``show`` / ``out_dir`` each image's map
also goes through the model's ``show_result`` (a colorized image, or the raw ``.npy`` under ``format_only``); with ``ply_dir`` it goes
through ``save_point_cloud`` (a coloured point cloud per image, a binary ``.ply``).

``device_eval=True`` (opt-in; the KITTI and the DDAD protocol) evaluates where the prediction is: every frame goes through the graphed
engine (apis/inference.py: flip-TTA for KITTI, the single view of DDADResize's shape for DDAD) and ``dataset.pre_eval_device_batch``
reduces its map to ten float64 sums on the engine's stream (csrc/eval.hip: ``ge_depth_metrics_batch`` or
``ge_depth_metrics_resized_batch``, with one frame); the whole split comes back in one copy at the end.  For DDAD the kernel
resamples the prediction at the ground-truth pixels in float32 (include/gedepth_ddad.h), which is not bit-equal to the host's
``F.interpolate``: the largest relative difference measured is 3.4e-7, so a threshold count can move by the pixels whose ratio lies that
close to 1.25^p.  ``show`` / ``out_dir`` and ``mask_pe`` are not covered.  ``eval_batch=F`` (2 .. 8) runs F frames per forward through the
batched engine (apis/batch_inference.py) and the same one call per batch, now with F frames, the next batch's image and ground-truth
PNGs decoding on a thread pool meanwhile; same rows, same tuples.  Either way the step behind a forward is ``_reduce``.  With DDAD the
batched engine is ``BatchDDADInferencer`` (every slot its own camera), the pool decodes the PNG and inflates the ground truth's ``.npz``, and ``ge_depth_metrics_resized_batch`` reduces the batch; the
rows carry the bits ``eval_batch=1`` gives the same maps.  Speed: README "KITTI speed" (KITTI) and "DDAD speed" (DDAD).

``strata=StrataSpec(...)`` (with ``device_eval``; KITTI protocol, any ``eval_batch``) adds one ``ge_depth_metrics_strata_batch`` call per
frame or batch behind the unchanged ``ge_depth_metrics_batch`` call, on the same stream and the same upload of the ground truth: the
ten sums per distance bin and on / off ground class (include/gedepth_strata.h), the ground plane being what the engine fed the front end
(``last_ground_depths`` of either engine).  Both buffers come back in the loop's one synchronisation and the loop returns
``(results, rows)``, ``rows`` (N, S, 10) float64; ``dataset.evaluate_strata`` prints the table.  Speed: README "Where the error is".

``errors=ErrorMaps(...)`` (with ``device_eval``; KITTI protocol, any ``eval_batch``, also with ``strata`` and ``ground_dir``) shows where in
the picture the error is (include/gedepth_error.h): behind the metric call, on the same upload of the ground truth, one
``ge_error_accumulate_batch`` call adds every return's abs-rel error into a per-pixel float64 sum and uint32 count held by ``errors``,
and with ``errors.out_dir`` one ``ge_error_image_batch`` call paints the batch's error pictures over the frames the front end was fed
(``last_frames`` of either engine).  A batch's pictures reach the host in one copy and are encoded on a thread pool while the next batch
computes; the planes come back in the loop's one synchronisation.  The loop returns what it returns without ``errors``.  Speed: README
"Where in the image the error is".

``ground_dir`` writes every image's ground maps (``DepthInferencer.ground_maps`` -> ``show_ground``: attention, slope and ground-depth
pictures, or one ``.npz`` under ``format_only``).  The maps exist on the engine's route only, so the frames go through the engine: alone
(no result list), or in the same pass as ``device_eval``; with the host loop's ``pre_eval`` it raises.  Speed: not measured.

``scene_dir`` (KITTI protocol) writes every image's scene cloud — the prediction, the ground prior, the LiDAR ground truth and the
slope-adjusted ground plane in one binary ``.ply`` (``DepthInferencer.scene_points`` -> ``write_scene_ply``) — through the engine, alone: it
returns no results and combines with no other output.  The loop: speed not measured; the kernel: README "Scene clouds".

``prior_sweep=PriorSweep(...)`` (with ``device_eval``; KITTI protocol, ``eval_batch=1``, alone) answers what the numbers do when the
calibration behind the ground prior is a little wrong: every frame runs ONCE through the batched engine with its V slots holding the
frame under V priors (``BatchDepthInferencer.sweep``: one ``ge_infer_front_sweep`` launch, include/gedepth_sweep.h) and ONE
``ge_depth_metrics_batch`` call reduces the V maps against one upload of the ground truth.  The loop returns ``(results, rows)``, ``rows``
(N, V, 10) float64; ``dataset.evaluate_sweep`` prints the table.  Speed: README "Prior sweep"."""
import os.path as osp

import numpy as np
import torch
import torch.distributed as dist

from ...mmrt.runner import get_dist_info


def _to_device(data, device):
    out = {}
    for k, v in data.items():
        if k == 'img_metas':
            out[k] = v
        elif isinstance(v, list):
            out[k] = [t.to(device, non_blocking=True) if torch.is_tensor(t) else t for t in v]
        else:
            out[k] = v.to(device, non_blocking=True) if torch.is_tensor(v) else v
    return out


def replace_str(s):
    """Output name of an image under ``out_dir`` (depth/apis/test.py of the reference): a leading '/' stripped, else '/' -> '_'."""
    if s[0] == '/':
        return s[1:]
    return s.replace('/', '_')


def _ply_file(depther, meta, depth, ply_dir):
    """``ply_dir/<ori_filename with .ply>``: the map's points through the image's ``cam_intrinsic`` meta, coloured from the frame's KB-crop
    window (the map is the bottom-aligned, horizontally centred window of the frame, as KBCrop cuts it)."""
    from .inference import _decode
    if 'cam_intrinsic' not in meta:
        raise KeyError('ply_dir: the test pipeline\'s Collect carries no cam_intrinsic meta (add LoadKITTICamIntrinsic and the meta key)')
    frame = _decode(meta['filename'])
    h, w = depth.shape[-2:]
    H, W = frame.shape[:2]
    if H < h or W < w:
        raise ValueError(f'ply_dir: the frame {(H, W)} is smaller than its map {(h, w)}: the map is not a crop of the frame')
    out_file = osp.join(ply_dir, osp.splitext(meta['ori_filename'])[0] + '.ply')
    depther.save_point_cloud(frame, [depth], meta['cam_intrinsic'], out_file, top=int(H - h), left=int((W - w) / 2))


def _show_batch(model, data, result_depth, show, out_dir, format_only, ply_dir=None):
    depther = getattr(model, 'module', model)
    for meta, depth in zip(data['img_metas'][0], result_depth):
        name = meta['ori_filename']
        if ply_dir:
            _ply_file(depther, meta, depth, ply_dir)
        if not (show or out_dir):
            continue
        if not out_dir:
            out_file = None
        elif format_only:
            out_file = osp.join(out_dir, name[:-4] + '.npy')
        else:
            out_file = osp.join(out_dir, replace_str(name))
        depther.show_result(name, [depth], show=show, out_file=out_file, format_only=format_only)


def _engine_frames(model, data_loader, what, evaluates=True, batch=1):
    """What the engine-backed loops share -> ``(depther, engine, indices in the sampler's order, their engine_frame arguments)``; every
    refusal is raised before the first frame runs, in the words of loop ``what``."""
    from ..datasets.pipelines import loading
    from .inference import _config_of, engine_for
    dataset = data_loader.dataset
    name, wants = type(dataset).__name__, getattr(dataset, 'device_protocol', None)
    if wants is None:
        raise NotImplementedError(f'{what}: {name} has no pre_eval_device (the KITTI and the DDAD protocol are evaluated on the device)')
    depther = getattr(model, 'module', model)
    if getattr(depther, 'cfg', None) is None:                            # this loop's own words for it
        raise NotImplementedError(f'{what}: model.cfg is missing (the engine reads the test protocol from it): build the model with '
                                  'init_depther or set model.cfg to its Config')
    spec, _ = config = _config_of(depther)                               # NotImplementedError names what the device front end lacks
    if spec['protocol'] != wants:                                        # before any attribute of the dataset is touched
        raise NotImplementedError(f'{what}: {name} is evaluated by the {wants} protocol, the model\'s test pipeline is the '
                                  f'{spec["protocol"]} protocol')
    if evaluates and wants == 'kitti' and (spec['height'], spec['width']) != (352, 1216):
        raise NotImplementedError(f'{what}: KBCrop {(spec["height"], spec["width"])}, the evaluation protocol crops (352, 1216)')
    bf16 = bool(torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == torch.bfloat16)      # what the caller asks for
    if batch != 1:
        from .batch_inference import check_batch
        check_batch(batch, spec, 'eval_batch', ddad=True)               # this loop has a batched engine for either protocol
    eng = engine_for(depther, bf16, config, batch)
    indices = [i for part in data_loader.batch_sampler for i in part]
    frames = [dataset.engine_frame(i) for i in indices]
    unknown = {f['camera'] for f in frames if 'camera' in f} - set(loading._DDAD_CAMERA_HEIGHT)       # DDAD; before the first frame runs
    if unknown:
        raise ValueError(f'{what}: the split holds frames of {", ".join(sorted(unknown))}; the cameras with '
                         f'a known height are {", ".join(sorted(loading._DDAD_CAMERA_HEIGHT))} (set the dataset\'s cameras to these)')
    return depther, eng, indices, frames


def _ground_file(dataset, index, ground_dir):
    """``ground_dir/replace_str(<the image's name in the split>)``: the name ``show_ground`` derives its files from."""
    return osp.join(ground_dir, replace_str(dataset.img_infos[index]['filename']))


def _ground_only(model, data_loader, ground_dir, format_only):
    """``ground_dir`` without an evaluation: every frame through ``DepthInferencer.ground_maps`` and ``show_ground``; no results."""
    depther, eng, indices, frames = _engine_frames(model, data_loader, 'ground_dir', evaluates=False)
    for i, frame in zip(indices, frames):
        depther.show_ground(eng.ground_maps(to_host=False, **frame), _ground_file(data_loader.dataset, i, ground_dir), format_only)
    return []


def _scene_only(model, data_loader, scene_dir):
    """``scene_dir``: every frame through ``DepthInferencer.scene_points`` with its ground truth, written as
    ``scene_dir/<ori_filename with .ply>``; no results."""
    from ..utils.point_cloud import write_scene_ply
    from .inference import SCENE_LAYERS, _config_of
    depther = getattr(model, 'module', model)
    if getattr(depther, 'cfg', None) is not None and _config_of(depther)[0]['protocol'] != 'kitti':
        raise NotImplementedError('scene_dir: the scene clouds are built for the KITTI protocol (a frame-sized ground prior and a uint16 '
                                  'ground truth in the KB-crop window)')
    depther, eng, indices, frames = _engine_frames(model, data_loader, 'scene_dir', evaluates=False)
    dataset = data_loader.dataset
    for i, frame in zip(indices, frames):
        out_file = osp.join(scene_dir, osp.splitext(dataset.img_infos[i]['filename'])[0] + '.ply')
        write_scene_ply(out_file, eng.scene_points(gt=dataset.gt_raw(i), **frame), SCENE_LAYERS)
    return []


class _ErrorPictures:
    """The error pictures' way from the device to ``out_dir``: per batch ONE copy of its pictures into a pinned host buffer on
    the engine's stream, with an event; when the loop has queued the next batch's device work, ``flush`` waits for the event (long
    reached), takes the pictures out of the pinned buffer — which is free for the next copy from then on — and hands their PNG encoding
    to a pool of ``DECODE_WORKERS`` threads, which runs while the device computes.  ``close`` writes the last batch and raises what an encoding raised."""

    def __init__(self, slots, device):
        from concurrent.futures import ThreadPoolExecutor
        from .batch_inference import DECODE_WORKERS
        self.device = device
        self.dev = torch.empty(slots, 352, 1216, 3, device=device, dtype=torch.uint8)          # what ge_error_image_batch writes
        self.host = torch.empty(slots, 352, 1216, 3, dtype=torch.uint8, pin_memory=True)
        # DECODE_WORKERS threads whatever the batch size: one picture takes longer to encode than one frame to compute, and the pictures
        # queue up behind the loop (at most MAX_QUEUED of them: then the loop waits for the oldest)
        self.pool = ThreadPoolExecutor(max_workers=DECODE_WORKERS)
        self.pending, self.futures = None, []

    MAX_QUEUED = 32

    def copy(self, n, files):
        """Queue the copy of the first ``n`` pictures of ``self.dev`` on the current stream; ``files``: where they go."""
        self.flush()                                                       # the last batch has left the pinned buffer
        self.host[:n].copy_(self.dev[:n], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.pending = (n, list(files), done)

    def flush(self):
        from ..models.depther.base import _imwrite_bgr
        if self.pending is None:
            return
        n, files, done = self.pending
        self.pending = None
        done.synchronize()
        pictures = self.host[:n].numpy().copy()                            # the pinned buffer is the next batch's again
        while len(self.futures) + n > self.MAX_QUEUED:
            self.futures.pop(0).result()                                   # raises what the encoding raised
        self.futures += [self.pool.submit(_imwrite_bgr, pictures[k], files[k]) for k in range(n)]

    def close(self):
        try:
            self.flush()
            for f in self.futures:
                f.result()
        finally:
            self.pool.shutdown(wait=True)


def _unpadded(n, total, rank, world):
    """How many of a rank's ``n`` sampler indices are the split's own: a non-shuffled DistributedSampler deals the indices round-robin
    (position ``k * world + rank`` for the rank's k-th) and pads the last round with the split's first entries when ``total % world != 0``;
    the positions from ``total`` on are that padding.  ``interleave_shards`` cuts it off the results; the error planes must never see it."""
    return sum(1 for k in range(n) if k * world + rank < total)


def _error_file(dataset, index, out_dir):
    """``out_dir/replace_str(<the image's name in the split>)``."""
    return osp.join(out_dir, replace_str(dataset.img_infos[index]['filename']))


def _strata_ground(eng, strata):
    """The ground depths the engine's front end was last fed, one per frame; None when ``strata`` has no ground class."""
    if not strata.ground:
        return None
    if eng.last_ground_depths is None:
        raise NotImplementedError('strata with spec.ground: the model\'s front end was fed no ground depth; use StrataSpec(ground=False)')
    return eng.last_ground_depths


def _reduce(dataset, eng, preds, indices, raws, row, sums, strata=None, rows=None, errors=None, pictures=None, real=None):
    """What follows a forward of either engine, on its stream: the n = ``len(indices)`` first maps of ``preds`` (F >= n, 1, H, W) fill
    rows ``row ..`` of ``sums`` (with ``strata`` also of ``rows``, from the ground depths the front end was fed; with ``errors`` the planes
    and pictures, from the frames it was fed: only the first ``real`` frames of the loop enter them), all on one upload of the ground
    truths (``raws``: decoded ahead, or None).  The pictures' copy to the host is queued behind."""
    n = len(indices)
    part = slice(row, row + n)
    with torch.cuda.stream(eng.stream):
        if errors is not None:
            count = min(max(real - row, 0), n)
            dataset.pre_eval_device_errors_batch(preds, indices, errors, eng.last_frames, pictures and pictures.dev, raws=raws,
                                                 sums_rows=sums[part], strata=strata, rows=None if strata is None else rows[part],
                                                 grounds=None if strata is None else _strata_ground(eng, strata), count=count)
            if pictures and count:
                pictures.copy(count, [_error_file(dataset, i, errors.out_dir) for i in indices[:count]])
        elif strata is None:
            dataset.pre_eval_device_batch(preds, indices, sums[part], raws=raws)
        else:
            dataset.pre_eval_device_strata_batch(preds, indices, rows[part], strata, _strata_ground(eng, strata), raws=raws,
                                                 sums_rows=sums[part])


def _device_eval_batches(dataset, eng, indices, frames, size, graph, **reduce):
    """``_device_eval``'s frames in batches of ``size``: the pool decodes the next batch's image and ground-truth PNGs while the batched
    engine and ``_reduce`` (its keyword arguments: ``reduce``) work on the current one; batch k fills rows ``k * size ..``."""
    from .batch_inference import decode_ahead
    from .inference import _decode
    jobs = [(lambda i=i, f=f: (_decode(f['img']), dataset.gt_raw(i))) for i, f in zip(indices, frames)]       # DDAD: the PNG and the .npz
    ddad = dataset.device_protocol == 'ddad'
    row = 0
    for decoded in decode_ahead(jobs, size):
        n = len(decoded)
        own = dict(cameras=[f['camera'] for f in frames[row:row + n]]) if ddad else {}       # each slot its camera's ground depth and height
        preds = eng.batch([d[0] for d in decoded], graph=graph, to_host=False, paths=[f['img'] for f in frames[row:row + n]], **own)
        _reduce(dataset, eng, preds, indices[row:row + n], [d[1] for d in decoded], row, **reduce)
        row += n


def _device_eval(model, data_loader, pre_eval, format_only, show, out_dir, ply_dir=None, ground_dir=None, eval_batch=1, engine_graph=True,
                 strata=None, errors=None):
    """The ``device_eval`` loop of ``single_gpu_test``: the list of metric tuples ``pre_eval`` yields, in the sampler's order.  Every
    forward is followed by ``_reduce``, with one frame (``eval_batch=1``: the single-frame engine, no pool) or with F.
    ``eval_batch=F > 1``: the sampler's indices in batches of F through the batched engine, image and ground-truth PNGs of the next
    batch decoding ahead; same rows of the same buffer, same one copy at the end.  ``strata`` (a ``core.StrataSpec``): every image's sums
    per stratum as well, into an (N, S, 10) buffer that comes back in the same synchronisation; the result is ``(the list, rows)``.
    ``errors`` (a ``core.ErrorMaps``): every image also goes into its error planes and, with its ``out_dir``, into an error picture
    (``pre_eval_device_errors_batch``, which then makes the metric and strata calls itself, on the same upload); the planes come back in
    the same synchronisation and the result is unchanged."""
    from ..core.evaluation import metrics_from_sums
    dataset = data_loader.dataset
    if not pre_eval or format_only:
        raise NotImplementedError('device_eval reduces every map to metric sums on the device: it needs pre_eval=True and no format_only')
    if show or out_dir or ply_dir:
        raise NotImplementedError('device_eval with show / out_dir / ply_dir: the depth maps never reach the host')
    if eval_batch != 1 and ground_dir:
        raise NotImplementedError('ground_dir with eval_batch > 1: the ground maps come from the single-frame engine; use eval_batch=1')
    depther, eng, indices, frames = _engine_frames(model, data_loader, 'device_eval', batch=eval_batch)
    sums = torch.empty(max(len(indices), 1), 10, device=eng.device, dtype=torch.float64)
    rows = None if strata is None else torch.empty(max(len(indices), 1), strata.count, 10, device=eng.device, dtype=torch.float64)
    pictures, real = None, len(indices)
    if errors is not None:
        rank, world = get_dist_info()
        real = _unpadded(len(indices), len(dataset), rank, world)      # a padded shard's last frame is the split's first again: keep it out
        errors.begin(eng.device, dataset.eval_rect(352, 1216))
        pictures = _ErrorPictures(eval_batch, eng.device) if errors.out_dir else None
    reduce = dict(sums=sums, strata=strata, rows=rows, errors=errors, pictures=pictures, real=real)
    try:
        if eval_batch != 1:
            _device_eval_batches(dataset, eng, indices, frames, eval_batch, engine_graph, **reduce)
        else:                                                          # one frame at a time: no pool, nothing decodes ahead
            for row, (i, frame) in enumerate(zip(indices, frames)):
                if ground_dir:
                    maps = eng.ground_maps(to_host=False, graph=engine_graph, **frame)
                    pred = maps['depth']
                else:
                    pred = eng(to_host=False, graph=engine_graph, **frame)
                _reduce(dataset, eng, pred[None], [i], None, row, **reduce)
                if ground_dir:
                    depther.show_ground(maps, _ground_file(dataset, i, ground_dir))
    finally:
        if pictures:
            pictures.close()
    with torch.cuda.stream(eng.stream):
        if strata is not None:
            host_rows = torch.empty(len(indices), strata.count, 10, dtype=torch.float64, pin_memory=True)
            host_rows.copy_(rows[:len(indices)], non_blocking=True)    # ordered before the copy below on the same stream
        if errors is not None:
            errors.download()                                          # the planes: ordered before the copy below, too
        host = sums[:len(indices)].cpu().numpy()                       # the one copy (and the one synchronisation) of the loop
    if errors is not None:
        errors.finish()
    torch.cuda.current_stream(eng.device).wait_stream(eng.stream)
    results = [metrics_from_sums(r) for r in host]
    return results if strata is None else (results, host_rows.numpy().copy())


def _sweep_refusals(prior_sweep, device_eval, eval_batch, strata, errors, ground_dir, scene_dir, data_loader):
    """What ``single_gpu_test(prior_sweep=...)`` refuses, before anything runs."""
    from ..core.evaluation import PriorSweep
    if not isinstance(prior_sweep, PriorSweep):
        raise TypeError(f'prior_sweep must be a depth.core.PriorSweep, got {type(prior_sweep).__name__}')
    if not device_eval:
        raise NotImplementedError('prior_sweep: the variants are the slots of the device evaluation loop\'s engine: it needs device_eval=True '
                                  '(the host loop is not covered)')
    if eval_batch != 1:
        raise NotImplementedError(f'prior_sweep with eval_batch={eval_batch}: the slots of a forward are the variants of ONE frame; use '
                                  'eval_batch=1')
    if strata is not None or errors is not None or ground_dir or scene_dir:
        raise NotImplementedError('prior_sweep with strata / errors / ground_dir / scene_dir: those read one prior per frame; run them apart')
    if getattr(data_loader.dataset, 'device_protocol', None) != 'kitti':
        raise NotImplementedError(f'prior_sweep: {type(data_loader.dataset).__name__} is not evaluated by the KITTI protocol (on DDAD the '
                                  'per-camera height also feeds the network, so the variants\' meaning needs its own decision)')


def _device_eval_sweep(model, data_loader, pre_eval, format_only, show, out_dir, ply_dir, engine_graph, sweep):
    """The ``prior_sweep`` loop of ``single_gpu_test``: per frame ONE ``BatchDepthInferencer.sweep`` (one decode, one upload, one front-end
    launch, one forward over the V = ``sweep.count`` variants) and ONE ``dataset.pre_eval_device_sweep`` (one upload of the ground truth,
    one ``ge_depth_metrics_batch`` call with V rows) into block ``row`` of an (N, V, 10) device buffer; the next frame's image and
    ground-truth PNGs decode ahead; one synchronising copy at the end -> ``(results, rows)``."""
    from ..core.evaluation import metrics_from_sums
    from .batch_inference import decode_ahead
    from .inference import _decode, sweep_slots
    dataset = data_loader.dataset
    if not pre_eval or format_only:
        raise NotImplementedError('device_eval reduces every map to metric sums on the device: it needs pre_eval=True and no format_only')
    if show or out_dir or ply_dir:
        raise NotImplementedError('device_eval with show / out_dir / ply_dir: the depth maps never reach the host')
    _, eng, indices, frames = _engine_frames(model, data_loader, 'prior_sweep', batch=sweep_slots(sweep))
    rows = torch.empty(max(len(indices), 1), sweep.count, 10, device=eng.device, dtype=torch.float64)
    jobs = [(lambda i=i, f=f: (_decode(f['img']), dataset.gt_raw(i))) for i, f in zip(indices, frames)]
    for row, ((bgr, raw),) in enumerate(decode_ahead(jobs, 1)):
        preds = eng.sweep(bgr, sweep, cam_height=sweep.cam_height, graph=engine_graph, to_host=False, path=frames[row]['img'])
        with torch.cuda.stream(eng.stream):
            dataset.pre_eval_device_sweep(preds, indices[row], rows[row], raw=raw)
    with torch.cuda.stream(eng.stream):
        host = rows[:len(indices)].cpu().numpy()                       # the one copy (and the one synchronisation) of the loop
    torch.cuda.current_stream(eng.device).wait_stream(eng.stream)
    return [metrics_from_sums(r) for r in host[:, 0]], host


def single_gpu_test(model, data_loader, pre_eval=False, format_only=False, format_args=None, device=None, *, show=False,
                    out_dir=None, device_eval=False, ply_dir=None, ground_dir=None, eval_batch=1, engine_graph=True, scene_dir=None,
                    strata=None, errors=None, prior_sweep=None):
    """Returns a list with one entry per image: the metric tuple (``pre_eval``) or the ``(1, H, W)`` depth map.  ``show`` / ``out_dir``:
    ``show_result`` of every image's map, written to ``out_dir/replace_str(ori_filename)`` (``format_only``: the raw map as
    ``out_dir/<ori_filename without extension>.npy``).  ``ply_dir``: every image's point cloud as ``ply_dir/<ori_filename with .ply>``
    (``save_point_cloud`` with the image's ``cam_intrinsic`` meta and its KB-crop offsets).  ``device_eval`` (with ``pre_eval``; KITTI or
    DDAD protocol): the module docstring.  ``ground_dir``: every image's ground maps (module docstring); without ``device_eval`` the
    result is an empty list.  ``eval_batch=F`` (2 .. 8; with ``device_eval``, KITTI or DDAD protocol, no ``ground_dir``): F frames per forward
    (``_device_eval``).  ``engine_graph=False``: the engine of ``device_eval`` runs eagerly and captures no hipGraph.  ``scene_dir`` (KITTI
    protocol; alone): every image's scene cloud as ``scene_dir/<ori_filename with .ply>`` (module docstring); the result is an empty list.
    ``strata`` (a ``core.StrataSpec``; with ``device_eval``, KITTI protocol, any ``eval_batch``): the loop also reduces every map to its
    metric sums per distance bin and on / off ground class (include/gedepth_strata.h) and returns ``(results, rows)``: ``results`` the list
    it returns without ``strata``, ``rows`` an (N, S, 10) float64 array in the same order (``dataset.evaluate_strata`` prints its table).
    ``errors`` (a ``core.ErrorMaps``; with ``device_eval``, KITTI protocol, any ``eval_batch``, also with ``strata`` and ``ground_dir``): the
    loop also adds every LiDAR return's abs-rel error into the per-pixel planes of ``errors`` and, with ``errors.out_dir``, writes every
    image's error picture to ``out_dir/replace_str(<name in the split>)`` (include/gedepth_error.h); the result is what the loop returns
    without ``errors``.  ``prior_sweep`` (a ``core.PriorSweep``; with ``device_eval``, KITTI protocol, ``eval_batch=1``, alone): every frame
    is evaluated under each of the sweep's V ground priors in one forward (``_device_eval_sweep``; include/gedepth_sweep.h) and the loop
    returns ``(results, rows)``: ``rows`` an (N, V, 10) float64 array of metric sums per image and variant (``dataset.evaluate_sweep``
    prints its table), ``results`` the tuples of ``rows[:, 0]``, the baseline, i.e. an ordinary result list."""
    model.eval()
    if prior_sweep is not None:
        _sweep_refusals(prior_sweep, device_eval, eval_batch, strata, errors, ground_dir, scene_dir, data_loader)
        return _device_eval_sweep(model, data_loader, pre_eval, format_only, show, out_dir, ply_dir, engine_graph, prior_sweep)
    if errors is not None:
        if not device_eval:
            raise NotImplementedError('errors: the error maps are reduced by the device evaluation loop: it needs device_eval=True (the host '
                                      'loop is not covered)')
        if getattr(data_loader.dataset, 'device_protocol', None) != 'kitti':
            raise NotImplementedError(f'errors: {type(data_loader.dataset).__name__} is not evaluated by the KITTI protocol (the error maps need '
                                      'its uint16 ground truth and its uint8 frame in the KB-crop window; the DDAD protocol is not covered)')
    if strata is not None:
        if not device_eval:
            raise NotImplementedError('strata are reduced by the device evaluation loop: it needs device_eval=True (the host loop is not covered)')
        if getattr(data_loader.dataset, 'device_protocol', None) != 'kitti':
            raise NotImplementedError(f'strata: {type(data_loader.dataset).__name__} is not evaluated by the KITTI protocol (the DDAD protocol\'s '
                                      'ge_depth_metrics_resized has no stratified form)')
    if scene_dir:
        if pre_eval or format_only or show or out_dir or ply_dir or ground_dir or device_eval or errors is not None:
            raise NotImplementedError('scene_dir with pre_eval / format_only / show / out_dir / ply_dir / ground_dir / device_eval / errors: the scene '
                                      'clouds come from an engine loop of their own that returns no results; run them apart')
        return _scene_only(model, data_loader, scene_dir)
    if eval_batch != 1 and not device_eval:
        raise NotImplementedError('eval_batch > 1 batches the device evaluation loop: it needs device_eval=True')
    if device_eval:
        return _device_eval(model, data_loader, pre_eval, format_only, show, out_dir, ply_dir, ground_dir, eval_batch, engine_graph, strata,
                            errors)
    if ground_dir:
        if pre_eval:
            raise NotImplementedError('ground_dir with the host loop\'s pre_eval: the ground maps exist on the engine\'s route only; '
                                      'evaluate with device_eval=True (tools/test.py: --device-eval) in the same pass')
        if show or out_dir or ply_dir:
            raise NotImplementedError('ground_dir with show / out_dir / ply_dir: those are outputs of the host loop; run them apart')
        return _ground_only(model, data_loader, ground_dir, format_only)
    dataset = data_loader.dataset
    if ply_dir:
        from ..datasets.ddad import DDADDataset
        if isinstance(dataset, DDADDataset):
            raise NotImplementedError('ply_dir on a DDAD split: DDADResize makes the map an area-resized view of the frame, not a crop of '
                                      'it, so no frame pixel colours a map pixel; depth.utils.depth_to_points with a caller-resized '
                                      'image serves DDAD maps')
    device = device or next(model.parameters()).device
    results = []
    for batch_indices, data in zip(data_loader.batch_sampler, data_loader):
        with torch.no_grad():
            result = model(return_loss=False, **_to_device(data, device))
        result_depth = list(result)                 # the maps, before format_results / pre_eval replace them
        if format_only:
            result = dataset.format_results(result, indices=batch_indices, **(format_args or {}))
        if pre_eval:
            result, _ = dataset.pre_eval(result, indices=list(batch_indices))
        results.extend(result)
        if show or out_dir or ply_dir:
            _show_batch(model, data, result_depth, show, out_dir, format_only, ply_dir)
    return results


def multi_gpu_test(model, data_loader, pre_eval=False, format_only=False, format_args=None, device=None, *, show=False, out_dir=None,
                   device_eval=False, ply_dir=None, ground_dir=None, eval_batch=1, engine_graph=True, scene_dir=None, strata=None,
                   errors=None, prior_sweep=None):
    """Each rank evaluates its shard of a non-shuffled DistributedSampler; rank 0 receives the results in dataset order.  ``show`` /
    ``out_dir`` / ``ply_dir`` / ``ground_dir`` / ``scene_dir`` / ``device_eval`` / ``eval_batch`` / ``engine_graph`` / ``strata`` as in
    ``single_gpu_test``: every rank writes the files of its own shard; with ``strata`` rank 0 receives ``(results, rows)``.  ``errors``:
    every rank writes its shard's pictures, and rank 0's ``errors`` receives the planes of all ranks, ``sum`` added in rank order, ``count``
    added exactly; the frames the sampler pads the last round with enter no plane and get no picture (``_unpadded``), so every image of
    the split is counted once.  ``prior_sweep`` raises: the sweep runs on one device (``single_gpu_test``)."""
    if prior_sweep is not None:
        raise NotImplementedError('multi_gpu_test(prior_sweep=...): the prior sweep runs on one device; use single_gpu_test')
    part = single_gpu_test(model, data_loader, pre_eval, format_only, format_args, device, show=show, out_dir=out_dir,
                           device_eval=device_eval, ply_dir=ply_dir, ground_dir=ground_dir, eval_batch=eval_batch, engine_graph=engine_graph,
                           scene_dir=scene_dir, strata=strata, errors=errors)
    rank, world = get_dist_info()
    if world == 1:
        return part
    if errors is not None:
        planes = [None] * world
        dist.all_gather_object(planes, (errors.sum, errors.count, errors.frames))
        if rank == 0:
            for s, c, f in planes[1:]:
                errors.add(s, c, f)
    gathered = [None] * world
    dist.all_gather_object(gathered, part)
    if rank != 0:
        return None
    total = len(data_loader.dataset)
    if strata is None:
        return interleave_shards(gathered, total)
    return interleave_shards([g[0] for g in gathered], total), interleave_shards([g[1] for g in gathered], total)


def interleave_shards(shards, total):
    """The shards of a non-shuffled DistributedSampler, which deals indices round-robin (shard k holds entries k, k + world, ...), back in
    dataset order, cut to ``total`` entries (the sampler pads the last round).  Lists give a list; arrays give an array stacked along axis 0."""
    ordered = []
    for i in range(max(len(g) for g in shards)):
        for g in shards:
            if i < len(g):
                ordered.append(g[i])
    ordered = ordered[:total]
    if shards and isinstance(shards[0], np.ndarray):
        return np.stack(ordered) if ordered else shards[0][:0]
    return ordered
