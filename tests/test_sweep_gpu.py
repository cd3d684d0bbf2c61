"""The prior sweep on the MI355X (csrc/infer.hip: ``ge_infer_front_sweep``; depth/apis/batch_inference.py: ``BatchDepthInferencer.sweep``;
depth/apis/test.py: ``single_gpu_test(prior_sweep=...)``; tools/test.py ``--prior-sweep``).

Kernel: slot v of one ``ge_infer_front_sweep`` launch against ``ge_infer_front`` on the plane tests/sweep_ref.py (numpy float32, no code
shared with the library) makes of the same ground depth — every byte, as uint32, so NaNs count — under red zones and poison
(tests/memguard.py).  Engine: ``sweep`` against ``batch`` fed the frame V times with the reference's planes: the static input bit for bit,
the maps within the bound tests/test_batch_gpu.py holds graph replay to (1e-6 of the map's largest value), eager and replayed, on ONE
capture; the forwards run under deterministic convolution algorithms.  Loop: the baseline rows against the plain ``device_eval`` loop at
``eval_batch=V`` (n and the threshold counts equal, the continuous sums within the engine's 2e-4), the other rows against ``ge_depth_metrics``
on the maps of ``inference_prior_sweep``, and the command line's file against the loop's rows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import memguard
import sweep_ref as R
import test_inference_gpu as TI
from toy_kitti import make_toy_kitti

pytestmark = pytest.mark.gpu

ROOT = TI.ROOT
MEAN = [float(np.float32(v)) for v in TI.MEAN]
STD = [float(np.float32(v)) for v in TI.STD]
ENGINE_EPS = 2e-4                                                    # the project's bound for the engine (tests/test_eval_device_gpu.py)
LIMITS = (256, 1e-3, 80)                                             # depth_scale, min_depth, max_depth of the KITTI evaluation
# (H, W, top, left, Hc, Wc): odd left (unaligned colour and plane reads) in a single block; left 4; 640 groups in several blocks
SHAPES = {'7x21': (7, 21, 2, 5, 5, 12), '11x40': (11, 40, 0, 4, 11, 36), '45x70': (45, 70, 5, 3, 40, 64)}
# n = 1: a negative c (q <= 0 beyond 100 m); n = 3: + the baseline and drop; n = 8: + a positive c, s of 0.5 and 2, c and s together, twice
VARIANTS = [(-0.01, 1.0, 0), (0.0, 1.0, 0), (0.0, 1.0, 1), (0.0125, 1.0, 0), (0.0, 0.5, 0), (0.0, 2.0, 0), (0.02, 1.5, 0), (-0.004, 0.75, 0)]


@functools.lru_cache(maxsize=None)
def _kernel_inputs(shape):
    """(bgr (H, W, 3) uint8, pe (H, W) float32): positives from 0.5 to 300 (some above pe_max = 200, many above 100 where c = -0.01 makes
    q <= 0), zeros, negatives, NaN (one with a payload) and +inf."""
    H, W = SHAPES[shape][:2]
    rng = np.random.default_rng(H * 100 + W)
    pe = rng.uniform(0.5, 300.0, (H, W)).astype(np.float32)
    kind = rng.integers(0, 12, (H, W))
    pe[kind == 0] = 0.0
    pe[kind == 1] = -rng.uniform(0.1, 50.0, int((kind == 1).sum())).astype(np.float32)
    pe[kind == 2] = np.nan
    pe[kind == 3] = np.inf
    flat = pe.reshape(-1)
    flat[np.flatnonzero(np.isnan(flat))[:1]] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]
    for k in range(4):
        assert (kind == k).any()
    assert (pe > 200).any() and ((pe > 100) & np.isfinite(pe)).any() and (pe < 1).any()
    return TI._frame(H + W, H, W), pe


@functools.lru_cache(maxsize=None)
def _kernel_refs(shape, views):
    """Per variant the (views, 5, Hc, Wc) images ``ge_infer_front`` writes for the reference's plane, as uint32: computed once."""
    from gedepth_amd import kernels as K
    H, W, top, left, Hc, Wc = SHAPES[shape]
    bgr, pe = _kernel_inputs(shape)
    d_bgr = torch.from_numpy(bgr).cuda()
    refs = []
    for c, s, drop in VARIANTS:
        plane = R.perturb(pe, c, s, drop)
        out = torch.empty(views, 5, Hc, Wc, device='cuda')
        K.infer_front(d_bgr, torch.from_numpy(plane).cuda(), out, top, left, MEAN, STD)
        refs.append(out.cpu().numpy().view(np.uint32))
    return refs


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('n', [1, 3, 8])
@pytest.mark.parametrize('views', [1, 2])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_sweep_slots_carry_the_bits_of_the_single_frame_kernel(monkeypatch, shape, views, n, poison):
    from gedepth_amd import hip, sweep_kernels
    from gedepth_amd import kernels as K
    H, W, top, left, Hc, Wc = SHAPES[shape]
    bgr, pe = _kernel_inputs(shape)
    refs = _kernel_refs(shape, views)
    guard = memguard.Guard(poison)
    guard.install(monkeypatch, [sweep_kernels], binding=hip)
    d_bgr, d_pe = guard.framed(torch.from_numpy(bgr).cuda()), guard.framed(torch.from_numpy(pe).cuda())
    out = guard.proxy.empty(views * (n + 1), 5, Hc, Wc, device='cuda', dtype=torch.float32)
    K.infer_front_sweep(d_bgr, d_pe, VARIANTS[:n], out, top, left, MEAN, STD, views=views)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()                                                     # the red zones of the frame, the plane and dst
    assert guard.launched == ['ge_infer_front_sweep']                 # one launch for the n variants
    got = out.cpu().numpy().view(np.uint32)
    for v in range(n):
        np.testing.assert_array_equal(got[views * v:views * v + views], refs[v], err_msg=f'{shape} views {views} variant {v} of {n}')
    assert bool(memguard.poisoned(out[views * n:], poison).all()), 'the images after the last variant must stay untouched'
    if n >= 2:                                                        # the baseline hands the plane through: channel 4 is the input's bits
        np.testing.assert_array_equal(got[views * 1, 4], pe[top:top + Hc, left:left + Wc].view(np.uint32))
    if n >= 3:
        assert not got[views * 2, 3:].any()                           # drop: both ground channels are +0


# ------------------------------------------------------------------------------------------------ the engine and the loop, on the toy tree
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('kitti_sweep'))
    return root, make_toy_kitti(root, seed=3)


@pytest.fixture(scope='module', autouse=True)
def _reproducible_convolutions():
    """As in test_ground_maps_gpu.py: with deterministic convolution algorithms the whole eval forward repeats its bits."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def _files(model):
    from gedepth_amd.depth.datasets import build_dataset
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    return ds, [os.path.join(ds.img_dir, info['filename']) for info in ds.img_infos]


@pytest.mark.parametrize('cfg_name', ['depthformer_swint_a.py', 'depthformer_swint_v.py'], ids=['adaptive', 'vanilla'])
def test_engine_sweep_equals_batch_on_the_reference_planes(tree, cfg_name):
    from gedepth_amd.depth.apis.inference import engine_for
    from gedepth_amd.depth.core import PriorSweep
    model = TI._model(cfg_name, *tree)
    _, files = _files(model)
    spec = PriorSweep(pitch_deg=(1.0,), drop=True)                    # V = 3: baseline, a pitch, no prior
    pe = np.load(os.path.join(tree[0], 'input', '2011_09_26', 'pe', 'pe_165.npy')).astype(np.float32)
    planes = [R.perturb(pe, *row) for row in spec.table()]
    assert not np.array_equal(planes[1], pe) and not planes[2].any()
    eng = engine_for(model, False, batch=4)                           # four slots, as the loop's sweep below: V = 3 leaves the last alone
    ref_maps = eng.batch([files[0]] * 3, pes=planes, graph=False)
    ref_in = eng.static_in.clone()
    eng.static_in.fill_(7.0)                                          # whatever sweep leaves alone shows
    maps = eng.sweep(files[0], spec, graph=False)
    assert torch.equal(eng.static_in[:6].view(torch.int32), ref_in[:6].view(torch.int32)), 'sweep and batch must feed the forward the same bits'
    assert bool((eng.static_in[6:] == 7.0).all()) and not ref_in[6:].any()       # the slot from V on keeps what it held
    assert len(eng.last_ground_depths) == len(eng.last_frames) == 3 == eng.last_n
    assert all(g is eng.last_ground_depths[0] for g in eng.last_ground_depths) and torch.equal(eng.last_ground_depths[0].cpu(), torch.from_numpy(pe))
    assert len(maps) == 3 and all(m.shape == (1, 352, 1216) and m.dtype == np.float32 for m in maps)
    for v, (m, r) in enumerate(zip(maps, ref_maps)):
        diff = np.abs(m - r).max()
        print(f'[{cfg_name} eager] variant {v}: |sweep - batch| max {diff:.2e} of {np.abs(r).max():.2f}')
        assert diff <= 1e-6 * np.abs(r).max(), v
    assert not np.array_equal(maps[0], maps[1]) and not np.array_equal(maps[0], maps[2])      # the prior reaches the map
    assert eng.captures == 0
    for _ in range(2):                                                # the warm-up calls under the key, then capture + replay
        eng.sweep(files[0], spec, graph=True)
    graphed = eng.sweep(files[0], spec, graph=True)
    assert eng.captures == 1 and eng.replays == 1
    for v, (g, m) in enumerate(zip(graphed, maps)):
        diff = np.abs(g - m).max()
        print(f'[{cfg_name} graph] variant {v}: |graph - eager| max {diff:.2e} of {np.abs(m).max():.2f}')
        assert diff <= 1e-6 * np.abs(m).max(), v
    again = eng.batch([files[0]] * 3, pes=planes, graph=True)         # batch replays sweep's capture: one graph for both
    assert eng.captures == 1 and eng.replays == 2 and len(eng.graphs) == 1
    for a, r in zip(again, ref_maps):
        assert np.abs(a - r).max() <= 1e-6 * np.abs(r).max()
    two = eng.sweep(files[1], spec.table()[:2], graph=True, to_host=False)       # V = 2 < F: the rows themselves, the device view
    assert tuple(two.shape) == (2, 1, 352, 1216) and two.data_ptr() == eng.static_out.data_ptr() and eng.last_n == 2
    with pytest.raises(ValueError, match='5 variants for an engine of 4 slots'):
        eng.sweep(files[0], PriorSweep(pitch_deg=(-1.0, 0.5, 1.0)))



def _assert_rows(got, ref, what, near=None):
    """n equal; the three threshold counts equal (``near``: within the pixels whose ratio lies within 2 * ENGINE_EPS of the threshold, the
    assertion of test_batch_gpu._assert_loop); each of the six continuous sums within the engine's 2e-4, relative."""
    assert got[0] == ref[0] > 1000, (what, got[0], ref[0])
    for k in range(3):
        assert abs(got[1 + k] - ref[1 + k]) <= (0 if near is None else near[k]), (what, k, got[1 + k], ref[1 + k], near)
    rel = [abs(got[k] - ref[k]) / abs(ref[k]) for k in range(4, 10)]
    print(f'[{what}] n {got[0]:.0f}, counts {got[1:4]} vs {ref[1:4]}, largest relative difference of a continuous sum {max(rel):.1e}')
    assert max(rel) <= ENGINE_EPS, (what, got, ref)


@pytest.fixture(scope='module')
def loop(tree):
    """(model, dataset, loader, files, the sweep, its (results, rows), per frame the V maps of ``inference_prior_sweep``) — the vanilla
    model with the kernel variants a fresh process runs (the command line's), V = 4, the engine run eagerly; computed once, left unchanged."""
    from gedepth_amd.depth.apis import inference_prior_sweep
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core import PriorSweep
    from gedepth_amd.depth.datasets import build_dataloader
    model = TI._model('depthformer_swint_v.py', *tree)
    for m in model.modules():
        if hasattr(m, 'kernel_variant'):
            m.kernel_variant = 0
    ds, files = _files(model)
    loader = lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False)      # noqa: E731
    spec = PriorSweep(pitch_deg=(-1.0, 1.0))
    results, rows = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, prior_sweep=spec, engine_graph=False)
    maps = [inference_prior_sweep(model, f, spec, graph=False) for f in files]
    return model, ds, loader, files, spec, results, rows, maps


def test_loop_baseline_rows_against_the_plain_device_loop(loop):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core import metrics_from_sums
    model, ds, loader, files, spec, results, rows, _ = loop
    assert spec.count == 4 and rows.shape == (4, 4, 10) and rows.dtype == np.float64 and len(results) == 4
    assert set(model._ge_inferencers) == {(False, 4)}                # the engine the plain loop runs at eval_batch = 4
    kept, plain_call = [], ds.pre_eval_device_batch

    def spy(preds, indices, sums_rows, raws=None):                    # the plain loop's sums, before metrics_from_sums folds them
        plain_call(preds, indices, sums_rows, raws=raws)
        kept.append(sums_rows)
    ds.pre_eval_device_batch = spy
    try:
        plain = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=4, engine_graph=False)
    finally:
        del ds.pre_eval_device_batch
    sums = torch.cat(kept).cpu().numpy()
    assert sums.shape == (4, 10) and len(plain) == 4
    for i in range(4):
        _assert_rows(rows[i, 0], sums[i], f'frame {i} baseline')
    for got, row in zip(results, rows[:, 0]):
        assert isinstance(got, tuple) and len(got) == 9
        np.testing.assert_array_equal(np.asarray(got), np.asarray(metrics_from_sums(row)))
    assert not np.array_equal(rows[:, 3], rows[:, 0]) and np.array_equal(rows[:, 3, 0], rows[:, 0, 0])      # 'no prior' moves the sums, not n
    table = ds.evaluate_sweep(rows, spec)
    assert list(table) == spec.names and all(np.isfinite(v) for entry in table.values() for v in entry.values())
    assert table['baseline']['abs_rel'] == pytest.approx(np.mean([r[3] for r in results]), rel=1e-12)


def test_loop_variant_rows_against_the_maps_of_inference_prior_sweep(loop):
    from gedepth_amd import kernels as K
    model, ds, _, files, spec, _, rows, maps = loop
    rect, limits = ds.eval_rect(352, 1216), (ds.depth_scale, ds.min_depth, ds.max_depth)
    for i in range(4):
        assert len(maps[i]) == 4 and all(m.shape == (1, 352, 1216) and m.dtype == np.float32 for m in maps[i])
        raw = ds.gt_raw(i)
        gt = torch.from_numpy(raw.copy()).cuda()                      # PIL's array is read-only
        for v in range(1, 4):
            out = torch.zeros(10, device='cuda', dtype=torch.float64)
            K.depth_metric_sums(torch.from_numpy(maps[i][v][0]).cuda(), gt, raw.shape[0] - 352, int((raw.shape[1] - 1216) / 2), rect, *limits, out)
            _assert_rows(rows[i, v], out.cpu().numpy(), f'frame {i} {spec.names[v]}')


def test_cli_prior_sweep_writes_the_rows(loop, tmp_path):
    """tools/test.py --prior-sweep --sweep-out in a fresh process, on a checkpoint of the loop's weights: the file's rows are the loop's.
    The process replays a captured graph from the third frame on and picks its convolution algorithms freely; the loop above ran eagerly
    under deterministic ones — both inside the engine's bound, so a threshold count may move by the pixels within 2 * ENGINE_EPS of it."""
    from gedepth_amd.mmrt.checkpoint import save_checkpoint
    model, ds, _, files, spec, _, rows, maps = loop
    ckpt, out = str(tmp_path / 'model.pth'), str(tmp_path / 'sub' / 'sweep.npz')
    save_checkpoint(model, ckpt)
    cfg = model.cfg.data.test
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'test.py'), os.path.join(TI.CFG, 'depthformer_swint_v.py'), ckpt, '--eval', 'x',
           '--synthetic', '0', '--device-eval', '--prior-sweep', '--sweep-pitch', '-1', '1', '--sweep-out', out, '--options',
           f'data.test.data_root={cfg.data_root}', f'data.test.split={cfg.split}', 'data.workers_per_gpu=0']
    r = subprocess.run(['timeout', '-k', '10', '600'] + cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        print('---- stdout ----\n' + r.stdout[-6000:] + '\n---- stderr ----\n' + r.stderr[-6000:])
    assert r.returncode == 0, r.returncode
    assert 'Prior sweep:' in r.stdout and 'no prior' in r.stdout and 'Summary:' in r.stdout
    got = np.load(out)
    assert sorted(got.files) == ['cam_height', 'height_scale', 'names', 'pitch_deg', 'rows']
    assert list(got['names']) == spec.names and list(got['pitch_deg']) == [-1.0, 1.0] and got['height_scale'].size == 0
    assert float(got['cam_height']) == 1.65 and got['rows'].shape == (4, 4, 10) and got['rows'].dtype == np.float64
    for i in range(4):
        gt = ds.eval_kb_crop(ds._gt(i))
        mask = ds.eval_mask(gt)
        for v in range(4):
            ratio = np.maximum(gt[mask] / maps[i][v][mask], maps[i][v][mask] / gt[mask])
            near = [int((np.abs(ratio - 1.25 ** p) <= 1.25 ** p * 2 * ENGINE_EPS).sum()) for p in (1, 2, 3)]
            _assert_rows(got['rows'][i, v], rows[i, v], f'command line, frame {i} {spec.names[v]}', near)
