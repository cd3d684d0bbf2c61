"""Batched KITTI inference and evaluation on the MI355X (csrc/infer.hip, csrc/eval.hip, gedepth_amd/batch_kernels.py,
depth/apis/batch_inference.py): the three batched entry points bit for bit against their single-frame counterparts under red zones and
poison (tests/memguard.py) — the same kernels at grid.y = n and at grid.y = 1, which checks the per-frame offsets — and against references
that share no code with them (the training pipeline's chain of aug.hip for the front end, the torch expression for the merge, float64
sums within the bounds of tests/test_eval_device_gpu.py for the metrics), the
batched engine against ``aug_test`` and against its own graph replay on a tree with two frame sizes, the batched device evaluation loop
against the host loop, and validation on the device while training.

Bounds.  Kernels: ``torch.equal`` (the metric rows as int64 views, so NaN rows compare); the metric rows against float64:
``test_eval_device_gpu._assert_sums``.  Engine against the host route: the project's
bound for the engine, max <= 2e-4 and mean <= 1e-5 relative per pixel (``ENGINE_EPS`` of tests/test_eval_device_gpu.py).  Graph replay
against the eager run: 1e-6 of the map's largest value (``test_inference_gpu.py::test_graph_replay``).  The loops: the assertions of
``test_eval_device_gpu.py::test_device_eval_loop_vs_host_loop`` — a count moves by at most the pixels whose ratio lies within 2 * ENGINE_EPS
of a threshold, the continuous metrics lie within ``_assert_tuple`` with ``_engine_extra``.

Measured (Swin-T, exact variants, batch=2): engine vs aug_test, largest relative difference 7.5e-06 over the five frames of two sizes
(vanilla) and 1.1e-05 over two frames (adaptive); graph replay vs eager at most 1.5e-05 of 43.7, i.e. 3.5e-07 of the map's largest value."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import memguard
import test_eval_device_gpu as TE
import test_inference_gpu as TI
from toy_kitti import make_toy_kitti

pytestmark = pytest.mark.gpu

MEAN = [float(np.float32(v)) for v in TI.MEAN]
STD = [float(np.float32(v)) for v in TI.STD]
SMALL = ((11, 30), (9, 27), (13, 33))                  # crop (8, 24): tops 3, 1, 5 and lefts 3, 1, 4
FRONT_CASES = {'small-3': ((8, 24), SMALL), 'small-1': ((8, 24), SMALL[1:2]), 'kitti-4': ((352, 1216), TI.KITTI_SIZES),
               'kitti-8': ((352, 1216), TI.KITTI_SIZES + TI.KITTI_SIZES[::-1])}


def _guard(monkeypatch, poison):
    from gedepth_amd import batch_kernels, hip
    guard = memguard.Guard(poison)
    monkeypatch.setattr(batch_kernels, '_WS', {})                    # a workspace cached by an earlier test would bypass the frames
    guard.install(monkeypatch, [batch_kernels], binding=hip)
    return guard


@functools.lru_cache(maxsize=None)
def _front_inputs(case):
    """Per frame (bgr uint8 (H, W, 3), raw ground depth f32 (H, W) with values below 0 and above the 200 m filter, top, left)."""
    (Hc, Wc), sizes = FRONT_CASES[case]
    out = []
    for k, (H, W) in enumerate(sizes):
        rng = np.random.default_rng(100 + k)
        pe = rng.uniform(-20.0, 260.0, (H, W)).astype(np.float32)
        out.append((TI._frame(40 + k, H, W), pe, H - Hc, int((W - Wc) / 2)))
    return out


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('views', [1, 2])
@pytest.mark.parametrize('case', list(FRONT_CASES))
def test_front_batch_equals_the_single_frame_kernel(monkeypatch, case, views, poison):
    from gedepth_amd import kernels as K
    (Hc, Wc), sizes = FRONT_CASES[case]
    frames = _front_inputs(case)
    n, slots = len(frames), len(frames) + 1
    refs = []
    for bgr, pe, top, left in frames:
        ref = torch.empty(views, 5, Hc, Wc, device='cuda')
        refs.append(K.infer_front(torch.from_numpy(bgr).cuda(), torch.from_numpy(pe).cuda(), ref, top, left, MEAN, STD))
    guard = _guard(monkeypatch, poison)
    bgrs = [guard.framed(torch.from_numpy(f[0]).cuda()) for f in frames]
    pes = [guard.framed(torch.from_numpy(f[1]).cuda()) for f in frames]
    out = guard.proxy.empty(views * slots, 5, Hc, Wc, device='cuda', dtype=torch.float32)
    K.infer_front_batch(bgrs, pes, out, [f[2] for f in frames], [f[3] for f in frames], MEAN, STD, views=views)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_infer_front_batch']                 # one launch for the n frames
    for f, ref in enumerate(refs):
        assert torch.equal(out[views * f:views * f + views], ref), (case, views, f)
    assert bool(memguard.poisoned(out[views * n:], poison).all()), 'the slot after the last frame must stay untouched'
    if views == 2:
        assert torch.equal(out[1], out[0].flip(-1))
    if case == 'small-3':                                             # the independent reference: the training pipeline's chain (aug.hip)
        for f, (bgr, pe, top, left) in enumerate(frames):
            chain = TI._chain(torch.from_numpy(bgr).cuda(), torch.from_numpy(pe).cuda(), top, left, Hc, Wc)      # pe_max, depth_scale: 200, as above
            for v in range(views):
                assert torch.equal(out[views * f + v], chain[v]), (case, views, f, v)


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('n,H,W', [(3, 5, 8), (4, 352, 1216)])
def test_merge_batch_equals_the_single_frame_kernel(monkeypatch, n, H, W, poison):
    from gedepth_amd import kernels as K
    g = torch.Generator(device='cuda').manual_seed(n)
    pred = torch.rand(2 * (n + 1), 1, H, W, device='cuda', generator=g) * 80.0
    refs = [K.tta_merge(pred[2 * f:2 * f + 2].contiguous()) for f in range(n)]
    guard = _guard(monkeypatch, poison)
    src = guard.framed(pred)
    out = guard.proxy.empty(n + 1, 1, H, W, device='cuda', dtype=torch.float32)
    K.tta_merge_batch(src, out, n)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_tta_merge_batch']
    for f in range(n):
        assert torch.equal(out[f], refs[f]) and torch.equal(out[f], (pred[2 * f] + pred[2 * f + 1].flip(-1)) / 2), f
    assert bool(memguard.poisoned(out[n], poison).all())


@functools.lru_cache(maxsize=None)
def _metric_frames(case):
    """Four (geom, raw, pred) with one crop size: aligned ground truth (W % 4 == 0, left % 4 == 0), unaligned, all-zero, and a fourth."""
    if case == 'one-block':                                          # crop (8, 24): the inputs of test_eval_device_gpu.py
        nan_geom, nan_raw, nan_pred = TE._nan_zero_inputs()
        aligned, unaligned = (9, 28, 1, 4, 8, 24), (11, 27, 3, 3, 8, 24)
        return [(aligned,) + TE._inputs(aligned, 21), (unaligned,) + TE._inputs(unaligned, 22), (aligned,) + TE._inputs(aligned, 23, 'zero'),
                (nan_geom, nan_raw, nan_pred)]
    aligned, unaligned, odd = (40, 532, 2, 8, 37, 516), (40, 530, 2, 9, 37, 516), (41, 531, 3, 12, 37, 516)       # ten workgroups per image
    return [(aligned,) + TE._inputs(aligned, 31), (unaligned,) + TE._inputs(unaligned, 32), (aligned,) + TE._inputs(aligned, 33, 'zero'),
            (odd,) + TE._inputs(odd, 34)]


def _metric_rect(case, Hc, Wc):
    return (1, Hc - 1, 3, Wc - 2) if case == 'multi-block' else (0, Hc, 0, Wc)


@functools.lru_cache(maxsize=None)
def _metric_refs(case):
    """Per image of ``_metric_frames(case)`` the ten float64 sums over the pixels that count: the reference of test_eval_device_gpu.py."""
    return [TE.R.sums_f64(*TE._host((geom, raw, pred, _metric_rect(case, *geom[4:])))) for geom, raw, pred in _metric_frames(case)]


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('case', ['one-block', 'multi-block'])
def test_metrics_batch_rows_carry_the_bits_of_the_single_image_kernel(monkeypatch, case, poison):
    from gedepth_amd import hip
    from gedepth_amd import kernels as K
    frames = _metric_frames(case)
    n = len(frames)
    Hc, Wc = frames[0][0][4:]
    assert all(f[0][4:] == (Hc, Wc) for f in frames) and Wc % 4 == 0
    rect = _metric_rect(case, Hc, Wc)
    pred = torch.from_numpy(np.stack([f[2] for f in frames])).cuda()
    ref = torch.zeros(n, 10, device='cuda', dtype=torch.float64)
    for f, (geom, raw, _) in enumerate(frames):
        K.depth_metric_sums(pred[f], torch.from_numpy(raw).cuda(), geom[2], geom[3], rect, *TE.LIMITS, ref[f])
    guard = _guard(monkeypatch, poison)
    d_pred = guard.framed(pred)
    gts = [guard.framed(torch.from_numpy(f[1]).cuda()) for f in frames]
    sums = guard.framed(torch.full((n + 2, 10), -7.0, device='cuda', dtype=torch.float64))
    K.depth_metric_sums_batch(d_pred, gts, [f[0][2] for f in frames], [f[0][3] for f in frames], rect, *TE.LIMITS, sums)
    K.depth_metric_sums_batch(d_pred, gts[:1], [frames[0][0][2]], [frames[0][0][3]], rect, *TE.LIMITS, sums[n + 1:])      # n = 1, the last row
    torch.cuda.synchronize()
    monkeypatch.undo()
    checked = guard.check()                                           # red zones of pred, the ground truths, the partials and the sums
    assert guard.launched == ['ge_depth_metrics_batch'] * 2 and 'ge_depth_metrics_batch_workspace' in guard.direct
    ws = [f for f in checked if os.path.basename(f.site[0]) == 'batch_kernels.py']
    assert len(ws) == 1 and ws[0].nbytes == hip.lib().ge_depth_metrics_batch_workspace(8, Hc, Wc)
    got = sums.cpu()
    assert torch.equal(got[:n].view(torch.int64), ref.cpu().view(torch.int64)), (got[:n], ref)
    assert bool((got[n] == -7.0).all()), 'the row after the last image must keep its value'
    assert torch.equal(got[n + 1].view(torch.int64), ref[0].cpu().view(torch.int64))
    for f, f64 in enumerate(_metric_refs(case)):                      # the independent reference: float64 sums, non-finite rows included
        TE._assert_sums(got[f].numpy(), f64, f'{case} image {f}')
    counts = got[:n, 0].tolist()
    assert counts[0] > 0 and counts[1] > 0 and counts[2] == 0 and not got[2].any()           # the all-zero ground truth counts nothing
    if case == 'one-block':
        assert bool(torch.isnan(got[3]).any())                        # the NaN / zero-prediction frame


# ------------------------------------------------------------------------------------------------ the engine, on a tree with two frame sizes
def _two_size_tree(root):
    """Three 375 x 1242 frames of 2011_09_26 and two 370 x 1224 frames of 2011_09_28, each date with its own pe_165.npy and ground truth."""
    rng = np.random.default_rng(17)
    lines = []
    for date, (H, W), count in (('2011_09_26', (375, 1242), 3), ('2011_09_28', (370, 1224), 2)):
        os.makedirs(os.path.join(root, 'input', date, 'pe'), exist_ok=True)
        np.save(os.path.join(root, 'input', date, 'pe', 'pe_165.npy'), TI._plane(H, W).astype(np.float64) * (1.0 if H == 375 else 1.1))
        d = f'{date}_drive_0001_sync'
        img_dir = os.path.join(root, 'input', date, d, 'image_02', 'data')
        gt_dir = os.path.join(root, 'gt_depth', d, 'proj_depth', 'groundtruth', 'image_02')
        os.makedirs(img_dir), os.makedirs(gt_dir)
        for f in range(count):
            name = f'{f:010d}.png'
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(img_dir, name))
            depth = np.where(rng.random((H, W)) < 0.05, rng.uniform(1.0, 80.0, (H, W)), 0.0)
            Image.fromarray((depth * 256).astype(np.uint16)).save(os.path.join(gt_dir, name))
            lines.append(f'{date}/{d}/image_02/data/{name} {d}/proj_depth/groundtruth/image_02/{name} 721.5377')
    split = os.path.join(root, 'split.txt')
    with open(split, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return split


def _host_maps(model, indices=None):
    """The host route for the frames of the model's test split: the host test pipeline and ``model(return_loss=False)`` (aug_test)."""
    from gedepth_amd.depth.apis.test import _to_device
    from gedepth_amd.depth.datasets import build_dataset
    from gedepth_amd.depth.datasets.loader import collate
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    indices = range(len(ds)) if indices is None else indices
    files, maps = [], []
    for i in indices:
        with torch.no_grad():
            maps.append(model(return_loss=False, rescale=True, **_to_device(collate([ds[i]]), 'cuda'))[0])
        files.append(os.path.join(ds.img_dir, ds.img_infos[i]['filename']))
    return files, maps


@pytest.fixture(scope='module')
def two_sizes(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('kitti_two_sizes'))
    return root, _two_size_tree(root)


@pytest.fixture(scope='module')
def vanilla(two_sizes):
    """(model, the five files in split order, the host route's maps, the batched engine's eager maps) — computed once, left unchanged."""
    from gedepth_amd.depth.apis import inference_depther
    model = TI._model('depthformer_swint_v.py', *two_sizes)
    files, host = _host_maps(model)
    assert [Image.open(f).size for f in files] == [(1242, 375)] * 3 + [(1224, 370)] * 2
    eager = inference_depther(model, files, batch=2, graph=False)
    return model, files, host, eager


def _assert_engine(got, host, what):
    assert len(got) == len(host)
    worst = 0.0
    for k, (g, h) in enumerate(zip(got, host)):
        assert isinstance(g, np.ndarray) and g.shape == (1, 352, 1216) and g.dtype == np.float32
        mx, mean = TI._rel(g, h)
        worst = max(worst, mx)
        print(f'[{what}] frame {k}: engine vs aug_test max {mx:.2e} mean {mean:.2e}')
        assert mx <= 2e-4 and mean <= 1e-5, (what, k, mx, mean)
    print(f'[{what}] largest relative difference over {len(got)} frames: {worst:.2e}')


def test_batched_engine_vs_aug_test_on_two_frame_sizes(vanilla):
    model, files, host, eager = vanilla
    _assert_engine(eager, host, 'vanilla batch=2')                  # five maps, in input order: the second batch mixes the two sizes
    eng = model._ge_inferencers[(False, 2)]
    assert eng.captures == 0 and eng.frames == 2 and eng.last_n == 1 and tuple(eng.static_in.shape) == (4, 5, 352, 1216)
    assert all(not np.array_equal(eager[a], eager[b]) for a in range(5) for b in range(a))
    from gedepth_amd.depth.apis.inference import engine_for
    assert engine_for(model, False) is engine_for(model, False, batch=1) is model._ge_inferencers[False]      # F = 1: the existing engine


def test_batched_engine_vs_aug_test_adaptive(two_sizes):
    from gedepth_amd.depth.apis import inference_depther
    model = TI._model('depthformer_swint_a.py', *two_sizes)
    files, host = _host_maps(model, (0, 3))                          # one frame of each size, in one batch
    _assert_engine(inference_depther(model, files, batch=2, graph=False), host, 'adaptive batch=2')


def test_batched_graph_replay(vanilla):
    from gedepth_amd.depth.apis import inference_depther
    model, files, _, eager = vanilla
    model._ge_inferencers.pop((False, 2))
    got = inference_depther(model, files, batch=2, graph=True)       # eager, eager, capture + replay of the batch with one real frame
    eng = model._ge_inferencers[(False, 2)]
    assert eng.captures == 1 and eng.replays == 1 and eng.last_n == 1 < eng.frames
    assert ('batch', 2) == eng._key()[-2:]
    for k, (g, e) in enumerate(zip(got, eager)):
        diff = np.abs(g - e).max()
        print(f'[batched graph] frame {k}: |graph - eager| max {diff:.2e} of {np.abs(e).max():.2f}')
        assert diff <= 1e-6 * np.abs(e).max(), k
    again = inference_depther(model, files[3:] + files[:1], batch=2, graph=True)     # replays only; a full batch after the partial one
    assert eng.captures == 1 and eng.replays == 3
    for g, e in zip(again, eager[3:] + eager[:1]):
        assert np.abs(g - e).max() <= 1e-6 * np.abs(e).max()


# ------------------------------------------------------------------------------------------------ the loops, on the toy tree
def _assert_loop(dev, host, ds, maps, what):
    """The assertions of ``test_eval_device_gpu.py::test_device_eval_loop_vs_host_loop`` for one pair of result lists."""
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    assert len(dev) == len(host) == len(maps) and all(isinstance(t, tuple) and len(t) == 9 for t in dev)
    for i, (d, h) in enumerate(zip(dev, host)):
        gt_m, pred_m = TE._counted(ds, i, maps[i])
        n = gt_m.size
        ratio = np.maximum(gt_m / pred_m, pred_m / gt_m)
        for k in range(3):
            near = int((np.abs(ratio - 1.25 ** (k + 1)) <= 1.25 ** (k + 1) * 2 * TE.ENGINE_EPS).sum())
            print(f'[{what} frame {i}] {METRIC_NAMES[k]}: device {d[k] * n:.0f} host {h[k] * n:.0f} of {n}, {near} pixels near the threshold')
            assert abs(round(d[k] * n) - round(h[k] * n)) <= near, (what, i, METRIC_NAMES[k], d[k] * n, h[k] * n, near)
            assert abs(d[k] * n - round(d[k] * n)) < 1e-6
        TE._assert_tuple(d, gt_m, pred_m, f'{what} frame {i}', extra=TE._engine_extra(gt_m, pred_m))


def _holds(*args):
    try:
        _assert_loop(*args)
    except AssertionError:
        return False
    return True


def _host_tuples(ds, maps):
    """What the host loop's ``pre_eval`` makes of the host route's maps: the tuples of ``single_gpu_test(pre_eval=True)``, without a second
    run of the model."""
    return [ds.pre_eval([m], [i])[0][0] for i, m in enumerate(maps)]


def _toy(root):
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    split = make_toy_kitti(root, seed=3)
    model = TI._model('depthformer_swint_v.py', root, split)
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    return model, ds, (lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False))


def test_batched_device_eval_loop_vs_host_loop(tmp_path):
    from gedepth_amd.depth.apis.test import single_gpu_test
    model, ds, loader = _toy(str(tmp_path))
    maps = single_gpu_test(model, loader())
    host = _host_tuples(ds, maps)
    batched = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=2)
    assert set(model._ge_inferencers) == {(False, 2)} and model._ge_inferencers[(False, 2)].captures == 0      # two batches: both eager
    _assert_loop(batched, host, ds, maps, 'eval_batch=2 vs host')
    single = single_gpu_test(model, loader(), pre_eval=True, device_eval=True)
    _assert_loop(batched, single, ds, maps, 'eval_batch=2 vs eval_batch=1')
    summary = ds.evaluate(batched)
    assert all(np.isfinite(v) for v in summary.values())
    with pytest.raises(NotImplementedError, match='ground_dir'):
        single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=2, ground_dir=str(tmp_path / 'g'))
    with pytest.raises(ValueError, match='1 .. 8'):
        single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=9)


def test_validation_on_the_device_while_training_sees_the_new_weights(tmp_path):
    """Three validations of two batches each during six iterations: eager, eager / capture + replay, replay / replay, replay.  The third is
    pure replay after two more optimizer steps: its tuples must be those of the FINAL weights (the host loop run afterwards), and must not
    be those of the initial weights.  lr = 1e-3 without warm-up: six AdamW steps move every weight by up to 6e-3, far beyond what the
    engine's 2e-4 bound could cover."""
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.apis.train import make_evaluate_fn, train_depther
    from gedepth_amd.depth.datasets.loader import SyntheticKITTI
    model, ds, loader = _toy(str(tmp_path / 'kitti'))
    maps0 = single_gpu_test(model, loader())
    host0 = _host_tuples(ds, maps0)
    cfg = model.cfg
    cfg.optimizer.lr = 1e-3
    cfg.lr_config = dict(policy='CosineAnnealing', min_lr_ratio=1e-8, by_epoch=False)        # no warm-up
    cfg.runner = dict(type='IterBasedRunner', max_iters=6)
    cfg.evaluation = dict(interval=2, by_epoch=False)
    cfg.checkpoint_config = cfg.log_config = None
    cfg.work_dir = str(tmp_path / 'work')
    cfg.data.samples_per_gpu, cfg.data.workers_per_gpu = 2, 0
    validations, modes = [], []
    evaluate, inner = ds.evaluate, make_evaluate_fn(ds, loader(), device_eval=True, eval_batch=2)
    ds.evaluate = lambda res, **kw: (validations.append(list(res)), evaluate(res, **kw))[1]

    def evaluate_fn(runner):
        out = inner(runner)
        modes.append(runner.model.training)
        return out
    model.train()
    train_depther(model, SyntheticKITTI(4, 128, 160, adaptive=False, seed=5), cfg, validate=True, evaluate_fn=evaluate_fn, logger=lambda m: None)
    ds.evaluate = evaluate
    eng = model._ge_inferencers[(False, 2)]
    assert len(validations) == 3 and modes == [True] * 3 and eng.captures == 1 and eng.replays == 4
    maps = single_gpu_test(model, loader())                           # the final weights, host route
    host = _host_tuples(ds, maps)
    _assert_loop(validations[2], host, ds, maps, 'third validation vs host loop at the final weights')
    assert not _holds(validations[2], host0, ds, maps0, 'third validation vs host loop at the INITIAL weights')
