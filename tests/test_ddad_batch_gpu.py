"""Batched DDAD evaluation on the MI355X: ``ge_infer_front_ddad_batch`` (csrc/infer.hip) and ``ge_depth_metrics_resized_batch`` (csrc/eval.hip)
under red zones and poison (tests/memguard.py), ``BatchDDADInferencer``, ``DDADDataset.pre_eval_device_batch`` and
``single_gpu_test(device_eval=True, eval_batch=F)`` on a six-frame toy DDAD tree of two cameras.

What pins a batched result is the single-frame entry point on the same frame (bit for bit: the same kernel, launched with one frame) and a
reference that shares no code with the launch path: the training kernels' composition for the front end, ``eval_ref.sums_f64`` on the float32
restatement of the resampling (tests/ddad_ref.py) for the sums, the single-frame engine and the host loop for engine and loop.  Helpers and
bounds are those of tests/test_ddad_device_gpu.py, imported."""
import os
import types

import numpy as np
import pytest
import torch

import ddad_ref as D
import eval_ref as R
import memguard
import test_ddad_device_gpu as T

pytestmark = pytest.mark.gpu

LIMITS, ENGINE_EPS = T.LIMITS, T.ENGINE_EPS
BAD_ARG, UNSUPPORTED = 10001, 10002
GEOMETRIES = {'integer': ((96, 160), (48, 80)), 'fractional': ((38, 61), (12, 20))}
MIXED = (((96, 160), (38, 61), (50, 77)), (12, 20))                     # one call whose slots differ in frame size and ground depth


# ------------------------------------------------------------------------------------------------ the front end
def _front_inputs(sizes, seed):
    rng = np.random.default_rng(seed)
    bgrs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
    pes = []
    for H, W in sizes:                                                  # every slot its own ground depth, with negatives and values beyond 250
        pe = rng.uniform(-20, 320, (H, W)).astype(np.float32)
        pe[0, 0], pe[-1, -1], pe[1, 1] = 250.0, 250.5, 0.0
        pes.append(pe)
    return bgrs, pes


def _front_case(monkeypatch, poison, sizes, shape, seed):
    from gedepth_amd import ddad_batch_kernels, hip, kernels
    n = len(sizes)
    mean, std = [float(np.float32(v)) for v in T.MEAN], [float(np.float32(v)) for v in T.STD]
    bgrs, pes = _front_inputs(sizes, seed)
    guard = memguard.Guard(poison)
    guard.install(monkeypatch, [ddad_batch_kernels], binding=hip)
    d_bgrs = [guard.framed(torch.from_numpy(b).cuda()) for b in bgrs]
    d_pes = [guard.framed(torch.from_numpy(p).cuda()) for p in pes]
    out = guard.proxy.empty(n + 1, 5, *shape, device='cuda', dtype=torch.float32)
    kernels.infer_front_ddad_batch(d_bgrs, d_pes, out, mean, std, True, 250.0, 250.0)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()                                                       # red zones of the frames, the ground depths and the output
    assert guard.launched == ['ge_infer_front_ddad_batch']
    assert bool(memguard.poisoned(out[n:], poison).all()), 'images beyond n must stay untouched'
    assert not bool(memguard.poisoned(out[:n], poison).any())
    single = torch.empty(1, 5, *shape, device='cuda')
    for f in range(n):
        kernels.infer_front_ddad(d_bgrs[f], d_pes[f], single, mean, std, True, 250.0, 250.0)
        assert torch.equal(out[f], single[0]), f'image {f} of {n}: not the bits of ge_infer_front_ddad'
        assert torch.equal(out[f], T._composition(d_bgrs[f], d_pes[f], *shape)), f'image {f} of {n}: not the bits of the training kernels'
        assert bool((out[f, 3] == 0).any()) and bool((out[f, 3] > 0).any()) and bool((out[f, 4] < 0).any()) and bool((out[f, 4] > 250).any())


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('n', [1, 3, 8])
def test_front_batch_vs_single_frame_and_training_kernels(monkeypatch, n, poison):
    for k, (frame, shape) in enumerate(GEOMETRIES.values()):
        _front_case(monkeypatch, poison, [frame] * n, shape, seed=10 * n + k)
    sizes, shape = MIXED
    _front_case(monkeypatch, poison, [sizes[f % len(sizes)] for f in range(max(n, 2))], shape, seed=10 * n + 7)


def test_front_batch_refusals():
    import ctypes
    from gedepth_amd import batch_kernels as B
    from gedepth_amd import hip
    lib = hip.lib()
    bgr = torch.zeros(38, 61, 3, device='cuda', dtype=torch.uint8)
    pe = torch.zeros(38 * 61 + 1, device='cuda')
    dst = torch.full((2 * 5 * 12 * 20 + 4,), -7.0, device='cuda')
    assert dst.data_ptr() % 16 == 0
    m = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)                      # noqa: E731

    def run(rows, n, out=dst.data_ptr(), Hd=12, Wd=20):
        return lib.ge_infer_front_ddad_batch(vp(B._table(rows)), n, out, Hd, Wd, 250.0, vp(m), vp(m), 250.0, 1, None)
    good = (bgr.data_ptr(), pe.data_ptr(), 38, 61, 0, 0)
    assert run([good] * 8, 0) == BAD_ARG and run([good] * 8, 9) == BAD_ARG
    assert run([good, (None,) + good[1:]], 2) == BAD_ARG and run([good, (good[0], None) + good[2:]], 2) == BAD_ARG
    assert run([good, good[:4] + (1, 0)], 2) == BAD_ARG and run([good, good[:4] + (0, 2)], 2) == BAD_ARG
    assert run([good] * 2, 2, Wd=18) == UNSUPPORTED and run([good] * 2, 2, out=dst.data_ptr() + 4) == UNSUPPORTED
    assert run([good] * 2, 2, Hd=39) == UNSUPPORTED and run([good, (good[0], pe.data_ptr() + 2) + good[2:]], 2) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all()), 'a refused call must launch nothing'
    assert run([good] * 2, 2) == 0                                      # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((dst[:2 * 5 * 12 * 20] != -7.0).all()) and bool((dst[2 * 5 * 12 * 20:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ the resized metric sums
KINDS = ('sparse', 'dense', 'zero')


def _sums_inputs(n, gt_shape, seed):
    """n predictions (12, 20) and ground truths of ``gt_shape`` whose kinds cycle; ONE slot (the last) holds a NaN and a 0 prediction."""
    preds = np.stack([T._pred(12, 20, seed + f) for f in range(n)])
    gts = [T._gt(*gt_shape, seed + f, KINDS[f % 3]) for f in range(n)]
    gts[n - 1] = T._gt(*gt_shape, seed + n - 1, 'dense')               # every tap of that slot's prediction reaches a counted pixel
    preds[n - 1, 3, 5], preds[n - 1, 9, 7] = np.nan, 0.0
    return preds, gts


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('gt_shape', [(36, 64), (37, 61)], ids=['float4', 'element'])
@pytest.mark.parametrize('n', [1, 2, 8])
def test_resized_batch_sums_under_guards(monkeypatch, n, gt_shape, poison):
    from gedepth_amd import ddad_batch_kernels, hip, kernels
    H, W = gt_shape
    preds, gts = _sums_inputs(n, gt_shape, seed=3 * n + W)
    guard = memguard.Guard(poison)
    monkeypatch.setattr(ddad_batch_kernels, '_WS', {})
    guard.install(monkeypatch, [ddad_batch_kernels], binding=hip)
    d_pred = guard.framed(torch.from_numpy(preds).cuda())
    d_gts = []
    for f, gt in enumerate(gts):
        if f == 0:                                                      # 4 bytes past a 16-byte boundary: the float4 decision differs per image
            flat = guard.framed(torch.from_numpy(np.concatenate(([0.0], gt.ravel())).astype(np.float32)).cuda())
            d_gts.append(flat[1:].view(H, W))
            assert d_gts[-1].data_ptr() % 16 == 4
        else:
            d_gts.append(guard.framed(torch.from_numpy(gt).cuda()))
            assert d_gts[-1].data_ptr() % 16 == 0
    sums = guard.proxy.empty(n + 2, 10, device='cuda', dtype=torch.float64)
    got = []
    for _ in range(2):
        kernels.depth_metric_sums_resized_batch(d_pred, d_gts, *LIMITS, sums[1:n + 1])
        torch.cuda.synchronize()
        got.append(sums.cpu().numpy()[1:n + 1].copy())
    monkeypatch.undo()
    frames = guard.check()                                              # red zones of pred, every gt, partials and sums
    assert guard.launched == ['ge_depth_metrics_resized_batch'] * 2 and guard.direct == ['ge_depth_metrics_resized_batch_workspace']
    assert got[0].tobytes() == got[1].tobytes(), 'two launches on the same input must give the same bits'
    ws = [f for f in frames if os.path.basename(f.site[0]) == 'ddad_batch_kernels.py']
    lib = hip.lib()
    assert len(ws) == 1 and ws[0].nbytes == lib.ge_depth_metrics_resized_batch_workspace(8, H, W)
    used = lib.ge_depth_metrics_resized_batch_workspace(n, H, W) // 8
    assert used == n * lib.ge_depth_metrics_resized_workspace(H, W) // 8
    stay = ws[0].poisoned()
    assert not bool(stay[:used].any()) and bool(stay[used:].all()), 'n images write the partials of n images'
    stay = memguard.poisoned(sums, poison).cpu().numpy()
    assert stay[0].all() and stay[-1].all() and not stay[1:-1].any(), 'rows next to the written ones must stay poisoned'
    single = torch.zeros(n, 10, device='cuda', dtype=torch.float64)
    for f in range(n):
        kernels.depth_metric_sums_resized(d_pred[f], d_gts[f], *LIMITS, single[f])
    single = single.cpu().numpy()
    for f in range(n):
        what = f'image {f} of {n}, gt {gt_shape}'
        assert got[0][f].tobytes() == single[f].tobytes(), (what, got[0][f], single[f])
        gt_m, pred_m = T._counted(preds[f], gts[f], D.resize_f32)
        T._assert_sums(got[0][f], R.sums_f64(gt_m, pred_m), what)
        assert (gt_m.size == 0) == (not gts[f].any())
    assert np.isnan(got[0][n - 1][4:]).any() and not np.isnan(got[0][:n - 1]).any(), 'the NaN prediction stays in its own row'


def test_resized_batch_refuses_mixed_ground_truth_sizes():
    from gedepth_amd import kernels
    pred = torch.ones(2, 12, 20, device='cuda')
    sums = torch.full((2, 10), -7.0, device='cuda', dtype=torch.float64)
    with pytest.raises(RuntimeError, match='unsupported'):
        kernels.depth_metric_sums_resized_batch(pred, [torch.ones(36, 64, device='cuda'), torch.ones(37, 61, device='cuda')], *LIMITS, sums)
    torch.cuda.synchronize()
    assert bool((sums == -7.0).all())
    kernels.depth_metric_sums_resized_batch(pred[:, None], [torch.ones(36, 64, device='cuda')] * 2, *LIMITS, sums)      # (F, 1, h, w) is taken
    assert sums.cpu().numpy()[:, 0].tolist() == [36 * 64] * 2


# ------------------------------------------------------------------------------------------------ engine and loop, on the toy tree
@pytest.fixture(scope='module')
def toy6(tmp_path_factory):
    """``toy`` of tests/test_ddad_device_gpu.py with three frames per camera: random-init depthformer_a_ddad.py at Swin-T width, 96 x 160
    frames, DDADResize to (48, 80); the config's cameras leave CAMERA_01 and CAMERA_05, the two of the tree with a known height."""
    from test_dataset_cpu import _make_toy_ddad
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    root = str(tmp_path_factory.mktemp('ddad_batch_eval'))
    split = _make_toy_ddad(root, frames=3, seed=7)
    cfg = Config.fromfile(os.path.join(T.CFG, 'depthformer_a_ddad.py'))
    swin_t, rev = [64, 96, 192, 384, 768], [768, 384, 192, 96, 64]
    cfg.model.pretrained = None
    cfg.model.backbone.update(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24])
    cfg.model.neck.update(in_channels=swin_t, out_channels=swin_t)
    cfg.model.pe_mask_neck.in_channels = rev
    cfg.model.dynamic_pe_neck.in_channels = rev
    cfg.model.decode_head.update(in_channels=swin_t, up_sample_channels=swin_t)
    cfg.data.test.pipeline = T._test_pipeline(os.path.join(root, 'pe'), (48, 80))
    cfg.data.test.split = split
    torch.manual_seed(0)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model.cfg = cfg
    model = T._exact_variants(model.cuda().eval())
    ds = build_dataset(cfg.data.test, dict(test_mode=True))
    assert [ds.camera_of(i) for i in range(len(ds))] == ['CAMERA_01'] * 3 + ['CAMERA_05'] * 3
    return model, ds, (lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False))


@pytest.fixture(scope='module')
def host_maps6(toy6):
    """The maps of the host loop (host test pipeline -> ``simple_test``), computed once."""
    from gedepth_amd.depth.apis.test import single_gpu_test
    model, ds, loader = toy6
    maps = single_gpu_test(model, loader())
    assert len(maps) == 6 and all(m.shape == (1, 48, 80) and m.dtype == np.float32 for m in maps)
    return maps


ORDER = ([0, 3, 1, 4], [2, 5])                                          # two batches of an F = 4 engine, cameras mixed; the last one short
FAR_HEIGHTS = {'CAMERA_01': 1.2, 'CAMERA_05': 2.2, 'CAMERA_06': 1.53, 'CAMERA_09': 1.53}      # 1 m apart, so that the height shows


def test_batch_engine_eager_vs_single_frame_engine(toy6, monkeypatch):
    """Every eager map of the F = 4 engine against the single-frame engine's eager map of that frame, per pixel and relative, within
    ``ENGINE_EPS`` (what is measured is the forward's own run-to-run difference and what the convolution library does differently at
    batch 4: test_ddad_device_gpu.py has the figures for batch 1; measured here on an MI355X: 3.8e-5 at most over the six frames).  The heights are set 1 m apart, as
    test_graph_replay_follows_the_camera_height does, so that a slot fed another camera's height would show: with the cameras swapped the
    same frames move by far more than the bound."""
    from gedepth_amd.depth.apis.batch_inference import BatchDDADInferencer
    from gedepth_amd.depth.apis.inference import DepthInferencer, _decode, engine_for
    from gedepth_amd.depth.datasets.pipelines import loading
    monkeypatch.setattr(loading, '_DDAD_CAMERA_HEIGHT', FAR_HEIGHTS)
    model, ds, _ = toy6
    files, cams = [i['filename'] for i in ds.img_infos], [ds.camera_of(i) for i in range(6)]
    single = DepthInferencer(model)
    ref = [single(f, graph=False) for f in files]
    eng = BatchDDADInferencer(model, 4)
    assert eng.static_in.shape == (4, 5, 48, 80) and eng.static_out.shape == (4, 1, 48, 80) and eng.static_height.shape == (4,)
    assert not bool(eng.static_in.any()) and bool(torch.isfinite(eng.static_height).all()) and bool((eng.static_height > 0).all())
    worst = 0.0
    for part in ORDER:
        got = eng.batch([files[i] for i in part], graph=False)          # the cameras from the paths
        assert len(got) == len(part) and eng.last_n == len(part) and eng.last_cameras == [cams[i] for i in part]
        for g, i in zip(got, part):
            assert g.shape == (1, 48, 80) and g.dtype == np.float32 and np.isfinite(g).all()
            assert torch.equal(eng.static_in[part.index(i)].cpu(), ds[i]['img'][0].float()), f'frame {i}: not the host pipeline\'s input'
            worst = max(worst, T._rel(g, ref[i]))
            print(f'[batch engine] frame {i} ({cams[i]}) in slot {part.index(i)}: eager vs single-frame engine {T._rel(g, ref[i]):.2e}')
    heights = eng.static_height.cpu().numpy()                           # the short batch filled slots 0 and 1; 2 and 3 keep the first batch's
    assert heights.tolist() == [np.float32(1.2), np.float32(2.2), np.float32(1.2), np.float32(2.2)]
    print(f'[batch engine] largest relative difference {worst:.2e} (bound {ENGINE_EPS:.0e})')
    assert eng.captures == 0 and worst <= ENGINE_EPS
    part = ORDER[0]
    swapped = eng.batch([files[i] for i in part], cameras=[cams[(i + 3) % 6] for i in part], graph=False)
    moved = [T._rel(s, ref[i]) for s, i in zip(swapped, part)]
    print(f'[batch engine] cameras swapped: the maps move by {min(moved):.2e} .. {max(moved):.2e} relative')
    assert min(moved) > 100 * ENGINE_EPS, 'each slot must get the height of its own camera'
    again = eng.batch([_decode(files[i]) for i in part], cameras=[cams[i] for i in part], graph=False)      # arrays, no paths
    assert max(T._rel(a, ref[i]) for a, i in zip(again, part)) <= ENGINE_EPS
    with pytest.raises(ValueError, match='5 frames for an engine of 4 slots'):
        eng.batch(files[:5], graph=False)
    with pytest.raises(ValueError, match='frames of'):
        eng.batch([np.zeros((100, 160, 3), np.uint8)], cameras=['CAMERA_01'], graph=False)
    with pytest.raises(ValueError, match='no camera for frame 0'):
        eng.batch([np.zeros((96, 160, 3), np.uint8)], graph=False)
    for name in ('points', 'ground_maps', 'scene_points', 'error_map', '__call__'):
        with pytest.raises(NotImplementedError):
            getattr(eng, name)(files[0])
    monkeypatch.undo()
    model.__dict__.pop('_ge_inferencers', None)
    assert isinstance(engine_for(model, batch=4), BatchDDADInferencer) and engine_for(model, batch=4) is engine_for(model, batch=4)
    out = engine_for(model, batch=4).run(files, graph=False)            # files to maps, the last batch short
    assert len(out) == 6 and all(o.shape == (1, 48, 80) and np.isfinite(o).all() for o in out)
    model.__dict__.pop('_ge_inferencers', None)


def test_batch_engine_replay_vs_eager(toy6):
    """Under reproducible convolutions a replayed batch equals its own eager run within the existing replay bound, 1e-6 of the map's
    maximum; one capture serves the full batches and the short last one."""
    from gedepth_amd.depth.apis.batch_inference import BatchDDADInferencer
    model, ds, _ = toy6
    files = [i['filename'] for i in ds.img_infos]
    full, short = ([files[i] for i in part] for part in ORDER)
    with T._reproducible_convolutions():
        eng = BatchDDADInferencer(model, 4)
        eager_full, eager_short = eng.batch(full, graph=False), eng.batch(short, graph=False)
        eng.batch(full), eng.batch(short)                               # the two warm-up batches
        assert eng.captures == 0
        replay_full = eng.batch(full)                                   # the capture, replayed
        assert eng.captures == 1 and eng.replays == 1
        replay_short = eng.batch(short)
        dev = eng.batch(full, to_host=False)
        assert dev.shape == (4, 1, 48, 80) and dev.data_ptr() == eng.static_out.data_ptr()
        torch.cuda.synchronize()
        assert eng.captures == 1 and eng.replays == 3 and list(eng.graphs) == [eng._key()] and eng._key()[-2:] == ('batch', 4)
    for name, eager, replay in (('full', eager_full, replay_full), ('short', eager_short, replay_short), ('device', eager_full, list(dev.cpu().numpy()))):
        assert len(eager) == len(replay)
        for f, (e, r) in enumerate(zip(eager, replay)):
            tol = 1e-6 * np.abs(e).max()
            print(f'[batch replay] {name} slot {f}: replay vs eager {np.abs(r - e).max():.2e} (tol {tol:.2e}), bit-identical {np.array_equal(r, e)}')
            assert np.abs(r - e).max() <= tol


def test_pre_eval_device_batch_on_the_maps_of_the_host_loop(toy6, host_maps6):
    """``pre_eval_device_batch`` fed device copies of the host loop's maps: every row carries the bits of ``pre_eval_device``."""
    model, ds, _ = toy6
    one = torch.full((7, 10), -7.0, device='cuda', dtype=torch.float64)
    for i, m in enumerate(host_maps6):
        ds.pre_eval_device(torch.from_numpy(m).cuda(), i, one[i])
    got = torch.full((7, 10), -7.0, device='cuda', dtype=torch.float64)
    maps = torch.from_numpy(np.stack(host_maps6)).cuda()
    assert maps.shape == (6, 1, 48, 80)
    ds.pre_eval_device_batch(maps[:4].contiguous(), [0, 1, 2, 3], got[0:4])
    ds.pre_eval_device_batch(maps[2:6].contiguous(), [4, 5], got[4:6], raws=[ds.gt_raw(4), ds.gt_raw(5)])      # F = 4 slots, n = 2
    one, got = one.cpu().numpy(), got.cpu().numpy()
    assert (got[6] == -7.0).all() and (one[6] == -7.0).all()
    # the second call read maps 2 and 3 for images 4 and 5: its rows are those of pre_eval_device on these maps
    two = torch.full((2, 10), -7.0, device='cuda', dtype=torch.float64)
    for k, i in enumerate((4, 5)):
        ds.pre_eval_device(maps[2 + k], i, two[k])
    assert got[:4].tobytes() == one[:4].tobytes() and got[4:6].tobytes() == two.cpu().numpy().tobytes()
    assert (got[:6, 0] > 1000).all()
    got_rows = torch.zeros(3, 10, device='cuda', dtype=torch.float64)
    with pytest.raises(ValueError, match='1 .. 8 images'):
        ds.pre_eval_device_batch(maps, [0, 1], got_rows)
    with pytest.raises(TypeError):
        ds.pre_eval_device_batch(maps.double(), [0, 1], got_rows[:2])
    with pytest.raises(TypeError):
        ds.pre_eval_device_batch(maps[:1], [0, 1], got_rows[:2])        # fewer maps than images


def _near(gt, pred):
    return [D.near_threshold(gt, pred, p, ENGINE_EPS) for p in (1, 2, 3)]


@pytest.fixture(scope='module')
def loops(toy6, host_maps6):
    """What the loop comparisons share, computed once: the host loop's tuples, the device loop's at ``eval_batch=1``, and per frame the
    counted ground truth with the host's resized prediction."""
    from gedepth_amd.depth.apis.test import single_gpu_test
    model, ds, loader = toy6
    host = single_gpu_test(model, loader(), pre_eval=True)
    model.__dict__.pop('_ge_inferencers', None)
    dev1 = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=1)
    counted = []
    for i in range(6):
        gt, mask = T._host_counted(ds, i)
        counted.append((gt[mask], ds.pre_eval([host_maps6[i]], [i])[1][0][0][mask]))
    return host, dev1, counted


def _assert_loop(dev, loops, what):
    """The tuples ``dev`` of a batched loop against the host loop and against ``eval_batch=1``, frame by frame."""
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    host, dev1, counted = loops
    assert len(dev) == len(host) == 6 and all(isinstance(t, tuple) and len(t) == 9 for t in dev)
    eps = ENGINE_EPS + D.HOST_BAND                                      # the continuous bound of test_device_eval_loop_vs_host_loop
    for i, (d, d1) in enumerate(zip(dev, dev1)):
        gt, pred = counted[i]
        n, near = gt.size, _near(gt, pred)
        print(f'[{what} frame {i}] {n} counted pixels, near the thresholds within {ENGINE_EPS:.0e}: {near}')
        # the allowance is a condition of this test: a wide band must not be able to hide a wrong count
        assert n > 1000 and sum(near) <= 0.01 * n, (what, i, near, n)
        T._assert_vs_host(d, gt, pred, f'{what} frame {i}', eps, band=ENGINE_EPS)          # n (integer counts), counts, continuous metrics
        extra = T._engine_extra(gt, pred, eps)
        for k, name in enumerate(METRIC_NAMES):
            if k < 3:
                assert abs(d[k] * n - round(d[k] * n)) < 1e-6 and abs(d1[k] * n - round(d1[k] * n)) < 1e-6          # the same n in both loops
                assert abs(round(d[k] * n) - round(d1[k] * n)) <= near[k], (what, i, name, d[k] * n, d1[k] * n, near[k])
            else:
                assert abs(d[k] - d1[k]) <= 2 * extra[name] + 1e-9, (what, i, name, d[k], d1[k])


@pytest.mark.parametrize('F', [2, 4])
def test_device_eval_loop_batched_vs_single_and_host(toy6, loops, F):
    """The test that fails without the feature: on the code before it, ``eval_batch > 1`` with a DDAD split raises NotImplementedError."""
    from gedepth_amd.depth.apis.batch_inference import BatchDDADInferencer
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    model, ds, loader = toy6
    model.__dict__.pop('_ge_inferencers', None)
    dev = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=F)
    eng = model._ge_inferencers[(False, F)]
    assert isinstance(eng, BatchDDADInferencer) and eng.frames == F
    assert eng.captures == (1 if F == 2 else 0) and eng.last_n == 2      # F = 2: three batches of two; F = 4: one full, one of two
    _assert_loop(dev, loops, f'eval_batch={F}')
    summary = ds.evaluate(dev)
    assert set(summary) == set(METRIC_NAMES) and all(np.isfinite(v) for v in summary.values())
    model.__dict__.pop('_ge_inferencers', None)


def test_make_evaluate_fn_runs_the_batched_loop(toy6, loops):
    """``make_evaluate_fn(device_eval=True, eval_batch=2)``, what tools/train.py validates through: the summary of that loop — every mean
    within what the per-frame bounds of ``_assert_loop`` allow against ``eval_batch=1`` — and the model back in training mode."""
    from gedepth_amd.depth.apis.train import make_evaluate_fn
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    model, ds, loader = toy6
    host, dev1, counted = loops
    model.__dict__.pop('_ge_inferencers', None)
    fn = make_evaluate_fn(ds, loader(), device_eval=True, eval_batch=2)
    try:
        summary = fn(types.SimpleNamespace(model=model))
        assert model.training
    finally:
        model.eval()
    assert (False, 2) in model._ge_inferencers and model._ge_inferencers[(False, 2)].captures == 1
    want = ds.evaluate(dev1)
    assert set(summary) == set(want) == set(METRIC_NAMES)
    eps = ENGINE_EPS + D.HOST_BAND
    for k, name in enumerate(METRIC_NAMES):
        if k < 3:
            bound = np.mean([_near(gt, pred)[k] / gt.size for gt, pred in counted])
        else:
            bound = np.mean([2 * T._engine_extra(gt, pred, eps)[name] + 1e-9 for gt, pred in counted])
        print(f'[make_evaluate_fn] {name}: eval_batch=2 {summary[name]!r} eval_batch=1 {want[name]!r} bound {bound:.1e}')
        assert abs(summary[name] - want[name]) <= bound + 1e-12, (name, summary[name], want[name], bound)
    model.__dict__.pop('_ge_inferencers', None)
