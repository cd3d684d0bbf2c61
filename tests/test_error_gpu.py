"""Error images and error planes on the MI355X (csrc/error.hip, include/gedepth_error.h, gedepth_amd/error_kernels.py) under red zones and
poison (tests/memguard.py), on the inputs of tests/error_cases.py (tests/test_error_cpu.py checks what they hold).

Bits: ``out`` and ``err`` equal the numpy restatement of tests/error_ref.py byte for byte (NaN positions of ``err`` compared apart); the
batch's blocks equal the single-image entry point's; the planes equal a sequential float64 sum in frame order.  Engine and loop run on
the toy tree with a toy model: the picture of ``error_map`` and every PNG of the loop decode to the restatement's image for the very map
the kernel was handed, and the loop's list is the plain loop's for those maps."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import error_cases as EC
import error_ref as ER
import memguard
from toy_kitti import make_toy_kitti

pytestmark = pytest.mark.gpu


def _install(monkeypatch, poison):
    from gedepth_amd import error_kernels, hip
    guard = memguard.Guard(poison)
    guard.install(monkeypatch, [error_kernels], binding=hip)
    return guard


def _same_plane(got, want):
    """float32 planes equal bit for bit where both are numbers, NaN in the same places."""
    got, want = np.asarray(got), np.asarray(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def _device_image(monkeypatch, poison, c, tau, radius, background, want_err=True):
    """``kernels.error_image`` on framed copies of the case's inputs -> (out, err) on the host; red zones and the launch record checked."""
    from gedepth_amd import kernels
    H, W, top, left, Hc, Wc = c['geom']
    guard = _install(monkeypatch, poison)
    d_pred, d_raw = guard.framed(torch.from_numpy(c['pred']).cuda()), guard.framed(torch.from_numpy(c['raw']).cuda())
    d_frame = None if background == 2 and poison == memguard.POISONS[1] else guard.framed(torch.from_numpy(c['frame']).cuda())
    out, err = kernels.error_image(d_pred, d_raw, d_frame, top, left, c['rect'], *c['limits'], tau, radius, background, want_err=want_err)
    torch.cuda.synchronize()
    monkeypatch.undo()
    frames = guard.check()                                            # red zones of pred, gt_raw, the frame, out and err
    assert guard.launched == ['ge_error_image']
    made = [f for f in frames if os.path.basename(f.site[0]) == 'error_kernels.py']
    assert len(made) == (2 if want_err else 1) and not any(bool(f.poisoned().any()) for f in made if f.dtype == torch.float32)
    return out.cpu().numpy(), None if err is None else err.cpu().numpy()


@pytest.mark.parametrize('background', [0, 1, 2])
@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('name', list(EC.CASES))
def test_image_equals_the_restatement_bit_for_bit(monkeypatch, name, radius, background):
    c = EC.CASES[name]
    want_out, want_err = EC.expected(name, radius, background)
    seen = []
    for poison in memguard.POISONS:
        out, err = _device_image(monkeypatch, poison, c, EC.TAU, radius, background)
        assert out.shape == want_out.shape and out.dtype == np.uint8 and np.array_equal(out, want_out), (name, radius, background, poison,
                                                                                                      np.argwhere((out != want_out).any(-1))[:8])
        assert err.dtype == np.float32 and _same_plane(err, want_err), (name, poison)
        seen.append(out)
    assert seen[0].tobytes() == seen[1].tobytes()                      # every byte was written: nothing of either poison is left


def test_image_without_the_err_plane(monkeypatch):
    c = EC.CASES['tiles-garg-aligned']
    out, err = _device_image(monkeypatch, memguard.POISONS[0], c, EC.TAU, 1, 1, want_err=False)
    assert err is None and np.array_equal(out, EC.expected('tiles-garg-aligned', 1, 1)[0])


def test_band_thresholds_on_the_device(monkeypatch):
    c = EC.threshold_case()
    want_out, want_err = ER.error_image(c['raw'], c['pred'], c['frame'], c['geom'], c['rect'], EC.THRESHOLD_TAU, 0, 2)
    n = want_err[0] / np.float32(EC.THRESHOLD_TAU)
    assert all(n[4 * j] == n[4 * j + 2] == np.float32(t) for j, t in enumerate(ER.T))       # host: every threshold is hit exactly
    out, err = _device_image(monkeypatch, memguard.POISONS[0], c, EC.THRESHOLD_TAU, 0, 2)
    assert np.array_equal(err, want_err) and np.array_equal(out, want_out)
    assert [tuple(p) for p in out[0, ::4]] == [tuple(ER.BGR[j + 1]) for j in range(9)]     # on the threshold: the upper band


def test_numpy_in_numpy_out():
    from gedepth_amd import kernels
    c = EC.CASES['one-tile-odd-left']
    H, W, top, left, Hc, Wc = c['geom']
    out, err = kernels.error_image(c['pred'], c['raw'], c['frame'], top, left, c['rect'], *c['limits'], EC.TAU, 1, 1)
    assert isinstance(out, np.ndarray) and isinstance(err, np.ndarray)
    want_out, want_err = EC.expected('one-tile-odd-left', 1, 1)
    assert np.array_equal(out, want_out) and _same_plane(err, want_err)
    s, n = np.zeros((Hc, Wc)), np.zeros((Hc, Wc), np.uint32)
    got = kernels.error_accumulate(c['pred'], c['raw'], top, left, c['rect'], *c['limits'], s, n)
    ws, wn = ER.accumulate([(c['raw'], c['pred'])], [c['geom']], c['rect'], (Hc, Wc))
    assert got[0] is s and got[1] is n and np.array_equal(s, ws) and np.array_equal(n, wn) and n.sum() > 0


# ------------------------------------------------------------------------------------------------ the batch entry point
BATCH_GEOMS = ((21, 44, 1, 4, 18, 40), (23, 43, 3, 3, 18, 40), (25, 52, 5, 8, 18, 40))       # vector loads, scalar loads, vector loads
BATCH_RECT = (2, 17, 3, 38)


def _batch_frames():
    """Three cases of different frame sizes and offsets on one (18, 40) crop."""
    return [EC.make_case(geom, BATCH_RECT, 60 + k) for k, geom in enumerate(BATCH_GEOMS)]


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('background', [1, 2])
def test_batch_blocks_carry_the_bytes_of_the_single_image_entry_point(monkeypatch, background, poison):
    from gedepth_amd import kernels as K
    cases = _batch_frames()
    n, (Hc, Wc) = len(cases), (18, 40)
    pred = torch.from_numpy(np.stack([c['pred'] for c in cases])).cuda()
    single = [K.error_image(pred[f], torch.from_numpy(c['raw']).cuda(), torch.from_numpy(c['frame']).cuda(), c['geom'][2], c['geom'][3],
                            BATCH_RECT, *ER.LIMITS, EC.TAU, 3, background) for f, c in enumerate(cases)]
    guard = _install(monkeypatch, poison)
    d_pred = guard.framed(pred)
    gts = [guard.framed(torch.from_numpy(c['raw']).cuda()) for c in cases]
    imgs = [guard.framed(torch.from_numpy(c['frame']).cuda()) for c in cases]
    if background == 2:
        imgs[1] = None                                                 # mixed null / non-null frames: allowed with background 2 only
    tops, lefts = [c['geom'][2] for c in cases], [c['geom'][3] for c in cases]
    out = guard.proxy.empty(n + 2, Hc, Wc, 3, device='cuda', dtype=torch.uint8)
    err = guard.proxy.empty(n + 2, Hc, Wc, device='cuda', dtype=torch.float32)
    K.error_image_batch(d_pred, gts, imgs, tops, lefts, BATCH_RECT, *ER.LIMITS, EC.TAU, 3, background, out=out, err=err)
    K.error_image_batch(d_pred, gts[:1], imgs[:1], tops[:1], lefts[:1], BATCH_RECT, *ER.LIMITS, EC.TAU, 3, background, out=out[n + 1:], err=err[n + 1:])
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_error_image_batch'] * 2
    for t in (out, err):
        stay = memguard.poisoned(t, poison).cpu().numpy()
        assert stay[n].all(), 'the block after the last image must stay poisoned'
    got_out, got_err = out.cpu().numpy(), err.cpu().numpy()
    for f, c in enumerate(cases):
        assert got_out[f].tobytes() == single[f][0].cpu().numpy().tobytes(), f
        assert got_err[f].tobytes() == single[f][1].cpu().numpy().tobytes(), f
        want_out, want_err = ER.error_image(c['raw'], c['pred'], c['frame'], c['geom'], BATCH_RECT, EC.TAU, 3, background)
        assert np.array_equal(got_out[f], want_out) and _same_plane(got_err[f], want_err), f      # the independent reference
    assert got_out[n + 1].tobytes() == got_out[0].tobytes() and got_err[n + 1].tobytes() == got_err[0].tobytes()
    if background != 2:
        with pytest.raises(ValueError, match='background=2'):
            K.error_image_batch(pred, gts, [imgs[0], None, imgs[2]], tops, lefts, BATCH_RECT, *ER.LIMITS, EC.TAU, 3, background)


# ------------------------------------------------------------------------------------------------ the accumulators
@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
def test_accumulate_equals_a_sequential_float64_sum(monkeypatch, poison):
    from gedepth_amd import kernels as K
    cases = _batch_frames()
    Hc, Wc = 18, 40
    rng = np.random.default_rng(5)
    sum0, count0 = rng.uniform(0.1, 3.0, (Hc, Wc)), rng.integers(1, 1000, (Hc, Wc)).astype(np.uint32)
    guard = _install(monkeypatch, poison)
    d_pred = guard.framed(torch.from_numpy(np.stack([c['pred'] for c in cases])).cuda())
    gts = [guard.framed(torch.from_numpy(c['raw']).cuda()) for c in cases]
    tops, lefts = [c['geom'][2] for c in cases], [c['geom'][3] for c in cases]
    d_sum, d_count = guard.framed(torch.from_numpy(sum0).cuda()), guard.framed(torch.from_numpy(count0.view(np.int32)).cuda()).view(torch.uint32)
    K.error_accumulate_batch(d_pred, gts[:2], tops[:2], lefts[:2], BATCH_RECT, *ER.LIMITS, d_sum, d_count)
    K.error_accumulate(d_pred[2], gts[2], tops[2], lefts[2], BATCH_RECT, *ER.LIMITS, d_sum, d_count)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_error_accumulate_batch', 'ge_error_accumulate']
    want_sum, want_count = ER.accumulate([(c['raw'], c['pred']) for c in cases], BATCH_GEOMS, BATCH_RECT, (Hc, Wc), sum0, count0)
    got_sum, got_count = d_sum.cpu().numpy(), d_count.view(torch.int32).cpu().numpy().view(np.uint32)
    assert got_sum.tobytes() == want_sum.tobytes()
    assert np.array_equal(got_count, want_count)
    masks = [ER.counted(c['raw'], c['geom'], BATCH_RECT)[1] for c in cases]
    errs = [ER.error_plane(c['raw'], c['pred'], c['geom'], BATCH_RECT) for c in cases]
    never = np.ones((Hc, Wc), bool)
    for m, e in zip(masks, errs):
        never &= ~(m & np.isfinite(e))
    odd = masks[0] & ~np.isfinite(errs[0]) & never                     # counted, but NaN or inf, and finite in no other frame
    assert odd.sum() >= 1 and np.array_equal(got_sum[never], sum0[never]) and np.array_equal(got_count[never], count0[never])
    assert (got_count > count0).sum() > 30


def test_wrapper_errors_on_the_device():
    from gedepth_amd import kernels
    pred, raw = torch.zeros(8, 20, device='cuda'), torch.zeros(11, 27, device='cuda', dtype=torch.uint16)
    frame = torch.zeros(11, 27, 3, device='cuda', dtype=torch.uint8)
    with pytest.raises(ValueError, match='leaves'):
        kernels.error_image(pred, raw, frame, 4, 3, (0, 8, 0, 20), *ER.LIMITS)               # the window leaves the frame
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.error_image(pred, raw, torch.zeros(11, 27, 3, dtype=torch.uint8), 3, 3, (0, 8, 0, 20), *ER.LIMITS)
    with pytest.raises(RuntimeError, match='unsupported'):
        kernels.error_image_batch(torch.zeros(1, 8, 22, device='cuda'), [raw], [frame], [3], [3], (0, 8, 0, 22), *ER.LIMITS)     # Wc % 4 != 0
    with pytest.raises(TypeError, match='float64'):
        kernels.error_accumulate(pred, raw, 3, 3, (0, 8, 0, 20), *ER.LIMITS, torch.zeros(8, 20, device='cuda'),
                                 torch.zeros(8, 20, device='cuda', dtype=torch.int32).view(torch.uint32))


# ------------------------------------------------------------------------------------------------ engine and loop, on the toy tree
@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    import test_inference_gpu as TI
    root = str(tmp_path_factory.mktemp('kitti_errors'))
    split = make_toy_kitti(root, seed=3)
    model = TI._model('depthformer_swint_v.py', root, split)
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    return model, ds, (lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False))


def _geom(raw):
    h, w = raw.shape
    return (h, w, h - 352, int((w - 1216) / 2), 352, 1216)


_DILATED = {}


def _reference_image(raw, pred, frame, rect, limits, tau, radius, background):
    """``error_ref.error_image`` at 352 x 1216 is a 428 000-window loop; the same maximum from the sparse returns instead (each return
    paints its own window, the larger n winning): the brute-force definition read from the sources' side."""
    geom = _geom(raw)
    H, W, top, left, Hc, Wc = geom
    err = ER.error_plane(raw, pred, geom, rect, limits)
    mask = ER.counted(raw, geom, rect, limits)[1]
    with np.errstate(all='ignore'):
        n = (err / np.float32(tau)).astype(np.float32)
    n[np.isnan(n)] = np.inf
    big = np.full((Hc, Wc), -1.0, np.float32)
    for r, c in zip(*np.nonzero(mask)):
        win = big[max(r - radius, 0):r + radius + 1, max(c - radius, 0):c + radius + 1]
        np.maximum(win, n[r, c], out=win)
    out = np.zeros((Hc, Wc, 3), np.uint8) if background == 2 else np.asarray(frame)[top:top + Hc, left:left + Wc].copy()
    if background == 1:
        out >>= 1
    out[big >= 0] = ER.BGR[ER.bands(big[big >= 0])]
    return out, err


def test_sparse_reference_is_the_brute_force_one():
    """A check of this file's own helper against tests/error_ref.py, not of the library: it needs no GPU and no feature to pass."""
    c = EC.CASES['tiles-and-remainders']
    H, W, top, left, Hc, Wc = c['geom']
    raw = np.zeros((375, 1242), np.uint16)
    pred = np.full((352, 1216), 7.0, np.float32)
    frame = np.zeros((375, 1242, 3), np.uint8)
    g = _geom(raw)
    raw[g[2]:g[2] + Hc, g[3]:g[3] + Wc] = c['raw'][top:top + Hc, left:left + Wc]
    pred[:Hc, :Wc] = c['pred']
    frame[g[2]:g[2] + Hc, g[3]:g[3] + Wc] = c['frame'][top:top + Hc, left:left + Wc]
    for radius in (0, 1, 3):
        got = _reference_image(raw, pred, frame, (0, Hc, 0, Wc), ER.LIMITS, EC.TAU, radius, 1)
        want = EC.expected('tiles-and-remainders', radius, 1)
        assert np.array_equal(got[0][:Hc, :Wc], want[0]) and _same_plane(got[1][:Hc, :Wc], want[1])


def test_engine_error_map_equals_the_restatement(toy):
    from gedepth_amd.depth.apis.inference import _decode, engine_for
    model, ds, _ = toy
    eng = engine_for(model)
    frame = ds.engine_frame(0)
    gt_path = os.path.join(ds.ann_dir, ds.img_infos[0]['ann']['depth_map'])
    rect = ds.eval_rect(352, 1216)
    head = model.decode_head
    for kw in (dict(), dict(tau=0.5, radius=3, background=0, rect=rect)):
        out, err = eng.error_map(frame['img'], gt_path, to_host=False, **kw)
        assert out.is_cuda and err.is_cuda and tuple(out.shape) == (352, 1216, 3) and tuple(err.shape) == (352, 1216)
        pred = eng.static_out.cpu().numpy()[0]
        want_out, want_err = _reference_image(np.asarray(Image.open(gt_path)), pred, _decode(frame['img']), kw.get('rect', (0, 352, 0, 1216)),
                                              (256.0, head.min_depth, head.max_depth), kw.get('tau', 0.05), kw.get('radius', 1),
                                              kw.get('background', 1))
        assert np.array_equal(out.cpu().numpy(), want_out) and _same_plane(err.cpu().numpy(), want_err)
        assert (want_err >= 0).sum() > 1000
    host = eng.error_map(frame['img'], ds.gt_raw(0))
    assert isinstance(host[0], np.ndarray) and host[0].dtype == np.uint8 and host[1].dtype == np.float32
    with pytest.raises(ValueError, match='gt has shape'):
        eng.error_map(frame['img'], np.zeros((10, 10), np.uint16))


def _plain_loop_on_the_same_maps(monkeypatch, ds):
    """Two runs of the forward differ in the last bits, so the loop with ``errors`` is compared with the plain loop on the very maps it
    was handed: the spy clones every prediction and also runs the plain metric call (``pre_eval_device`` / ``pre_eval_device_batch`` with
    the same arguments) on it into a buffer of this test; ``tuples()`` is the list the loop without ``errors`` returns for these maps."""
    from gedepth_amd.depth.core import metrics_from_sums
    sums = torch.zeros(len(ds), 10, device='cuda', dtype=torch.float64)
    seen, maps = [], []
    single, batch = ds.pre_eval_device_errors, ds.pre_eval_device_errors_batch

    def spy_single(pred, index, errors, frame, out=None, raw=None, **kw):
        ds.pre_eval_device(pred, index, sums[len(seen)])
        seen.append(index)
        maps.append(pred.clone())
        return single(pred, index, errors, frame, out, raw, **kw)

    def spy_batch(preds, indices, errors, frames, outs=None, raws=None, **kw):
        ds.pre_eval_device_batch(preds, indices, sums[len(seen):len(seen) + len(indices)], raws=raws)
        seen.extend(indices)
        maps.extend(p.clone() for p in preds[:len(indices)])
        return batch(preds, indices, errors, frames, outs, raws, **kw)
    monkeypatch.setattr(ds, 'pre_eval_device_errors', spy_single, raising=False)
    monkeypatch.setattr(ds, 'pre_eval_device_errors_batch', spy_batch, raising=False)
    return seen, maps, lambda: [metrics_from_sums(r) for r in sums.cpu().numpy()]


def test_loop_returns_the_plain_results_pictures_and_planes(toy, monkeypatch, tmp_path):
    from gedepth_amd.depth.apis.inference import _decode
    from gedepth_amd.depth.apis.test import replace_str, single_gpu_test
    from gedepth_amd.depth.core import ErrorMaps
    model, ds, loader = toy
    rect, limits = ds.eval_rect(352, 1216), (ds.depth_scale, ds.min_depth, ds.max_depth)
    counted = sum(int(ds.eval_mask(ds.eval_kb_crop(ds._gt(i))).sum()) for i in range(len(ds)))
    for F in (1, 2):
        out_dir = str(tmp_path / f'pictures{F}')
        errors = ErrorMaps(out_dir)
        seen, maps, tuples = _plain_loop_on_the_same_maps(monkeypatch, ds)
        results = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=F, errors=errors)
        monkeypatch.undo()
        plain = tuples()
        assert seen == list(range(len(ds))) and isinstance(results, list) and results == plain, (F, results, plain)
        assert errors.frames == len(ds) and errors.rect == tuple(rect)
        assert errors.sum.dtype == np.float64 and errors.count.dtype == np.uint32 and errors.sum.shape == errors.count.shape == (352, 1216)
        frames = []
        for i, pred in zip(seen, maps):
            raw, p = ds.gt_raw(i), pred.cpu().numpy()[0]
            frames.append((raw, p))
            want, _ = _reference_image(raw, p, _decode(ds.engine_frame(i)['img']), rect, limits, 0.05, 1, 1)
            png = os.path.join(out_dir, replace_str(ds.img_infos[i]['filename']))
            assert np.array_equal(np.asarray(Image.open(png))[..., ::-1], want), (F, i)
        assert len(os.listdir(out_dir)) == len(ds)
        assert int(errors.count.sum()) == counted > 1000               # exact, and independent of the prediction
        want_sum, want_count = ER.accumulate(frames, [_geom(f[0]) for f in frames], rect, (352, 1216), limits=limits)
        assert errors.sum.tobytes() == want_sum.tobytes() and np.array_equal(errors.count, want_count)
        save = str(tmp_path / f'summary{F}')
        errors.save(save)
        z = np.load(os.path.join(save, 'summary.npz'))
        assert np.array_equal(z['sum'], errors.sum) and np.array_equal(z['count'], errors.count) and float(z['tau']) == 0.05
        assert tuple(z['rect']) == tuple(rect) and Image.open(os.path.join(save, 'mean_abs_rel.png')).size == (1216, 352)
        mean, count = errors.rows(8)
        assert count.sum() == counted and np.isfinite(mean[count > 0]).all()


def test_loop_keeps_a_padded_shard_out_of_planes_and_pictures(toy, monkeypatch, tmp_path):
    """As rank 1 of 3 the loader's four indices stand at positions 1, 4, 7, 10 of the padded sampler: only the first is the split's own.
    All four frames are evaluated (the shard's results are cut later), one enters the planes and gets a picture; F = 2 splits a batch."""
    from gedepth_amd.depth.apis import test as T
    from gedepth_amd.depth.core import ErrorMaps
    model, ds, loader = toy
    first = int(ds.eval_mask(ds.eval_kb_crop(ds._gt(0))).sum())
    monkeypatch.setattr(T, 'get_dist_info', lambda: (1, 3))
    for F in (1, 2):
        out_dir = str(tmp_path / f'padded{F}')
        errors = ErrorMaps(out_dir)
        results = T.single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=F, errors=errors)
        assert len(results) == len(ds) == 4 and all(np.isfinite(r[3]) for r in results)
        assert errors.frames == 1 and int(errors.count.sum()) == first > 1000 and int(errors.count.max()) == 1
        assert os.listdir(out_dir) == [T.replace_str(ds.img_infos[0]['filename'])]


def test_loop_combines_with_strata_and_skips_pictures_without_out_dir(toy, monkeypatch):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core import ErrorMaps, StrataSpec
    model, ds, loader = toy
    counted = sum(int(ds.eval_mask(ds.eval_kb_crop(ds._gt(i))).sum()) for i in range(len(ds)))
    errors, spec = ErrorMaps(), StrataSpec()
    seen, maps, tuples = _plain_loop_on_the_same_maps(monkeypatch, ds)
    results, rows = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=2, strata=spec, errors=errors)
    monkeypatch.undo()
    assert results == tuples() and rows.shape == (len(ds), spec.count, 10)
    assert int(errors.count.sum()) == counted == int(rows[..., 0].sum())
