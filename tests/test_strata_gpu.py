"""Stratified metric sums on the MI355X (csrc/eval.hip, include/gedepth_strata.h, gedepth_amd/strata_kernels.py) under red zones and poison
(tests/memguard.py), on the inputs of tests/strata_cases.py (tests/test_strata_cpu.py checks what they hold).

Bits: row s is byte-equal to ``kernels.depth_metric_sums`` on the same prediction with the ground truth zeroed outside stratum s, the mask
taken from tests/strata_ref.py; with no edges and no ground plane the one row is ``depth_metric_sums``' own.  Values: every row against the
float64 restatement within the bounds of tests/test_eval_device_gpu.py ``_assert_sums`` (counts equal; 1e-12 relative, 1e-9 for the three
sums with a logarithm).  Batch: each image's block byte-equal to the single-image entry point's.  Loop: ``single_gpu_test(strata=...)`` on
a toy tree whose ground truth follows the ground plane for about half of the returns below the horizon; the per-stratum pixel counts do
not depend on the prediction and must equal the restatement's."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import memguard
import strata_cases as SC
import strata_ref as SR
import test_eval_device_gpu as TE
from toy_kitti import make_toy_kitti

pytestmark = pytest.mark.gpu
LIMITS = TE.LIMITS


def _install(monkeypatch, poison):
    from gedepth_amd import eval_kernels, hip, strata_kernels
    guard = memguard.Guard(poison)
    for mod, names in ((eval_kernels, ('_WS',)), (strata_kernels, ('_WS', '_WS_BATCH'))):
        for name in names:
            monkeypatch.setattr(mod, name, {})                          # a workspace cached by an earlier test would bypass the frames
    guard.install(monkeypatch, [eval_kernels, strata_kernels], binding=hip)
    return guard


def _framed_ground(guard, ground, offset):
    """The plane inside a frame; ``offset`` = 1: it starts one element into its buffer (4-byte aligned only) and ends where the buffer ends."""
    if ground is None:
        return None
    if not offset:
        return guard.framed(torch.from_numpy(ground).cuda())
    flat = guard.framed(torch.cat([torch.zeros(offset), torch.from_numpy(ground).flatten()]).cuda())
    return flat[offset:].view(ground.shape)


def _device_strata(monkeypatch, poison, c, edges, ground, launches=2):
    """``launches`` runs of kernels.depth_metric_sums_strata into blocks 1.. of a framed (launches + 2, S, 10) buffer; inputs and workspace
    framed too."""
    from gedepth_amd import hip, kernels
    geom, S = c['geom'], SR.count(edges, ground)
    guard = _install(monkeypatch, poison)
    d_pred, d_raw = guard.framed(torch.from_numpy(c['pred']).cuda()), guard.framed(torch.from_numpy(c['raw']).cuda())
    d_ground = _framed_ground(guard, ground, c['ground_offset'])
    assert d_ground is None or d_ground.data_ptr() % 16 == (4 * c['ground_offset']) % 16
    rows = guard.proxy.empty(launches + 2, S, 10, device='cuda', dtype=torch.float64)
    for k in range(launches):
        kernels.depth_metric_sums_strata(d_pred, d_raw, geom[2], geom[3], c['rect'], *LIMITS, rows[1 + k], edges, d_ground, c['tol'])
    torch.cuda.synchronize()
    monkeypatch.undo()
    frames = guard.check()                                            # red zones of pred, gt_raw, ground, partials and sums
    assert guard.launched == ['ge_depth_metrics_strata'] * launches and 'ge_depth_metrics_strata_workspace' in guard.direct
    ws = [f for f in frames if os.path.basename(f.site[0]) == 'strata_kernels.py']
    assert len(ws) == 1 and ws[0].nbytes == hip.lib().ge_depth_metrics_strata_workspace(1, geom[4], geom[5], S) and not bool(ws[0].poisoned().any())
    stay = memguard.poisoned(rows, poison).cpu().numpy()
    assert stay[0].all() and stay[-1].all() and not stay[1:-1].any(), 'blocks next to the written ones must stay poisoned'
    return rows.cpu().numpy()[1:-1]


def _plain_sums(c, raw):
    """``kernels.depth_metric_sums`` on the case's prediction and this ground truth."""
    from gedepth_amd import kernels
    out = torch.zeros(10, device='cuda', dtype=torch.float64)
    kernels.depth_metric_sums(torch.from_numpy(c['pred']).cuda(), torch.from_numpy(raw).cuda(), c['geom'][2], c['geom'][3], c['rect'], *LIMITS, out)
    return out.cpu().numpy()


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('name', list(SC.CASES))
def test_rows_carry_the_bits_of_the_plain_sums_on_a_masked_ground_truth(monkeypatch, name, poison):
    c = SC.CASES[name]
    got = _device_strata(monkeypatch, poison, c, c['edges'], c['ground'])
    assert got[0].tobytes() == got[1].tobytes(), 'two launches on the same input must give the same bits'
    for s in range(c['S']):
        masked = SR.raw_of_stratum(c['raw'], c['ground'], c['geom'], c['rect'], c['edges'], c['tol'], s)
        assert got[0][s].tobytes() == _plain_sums(c, masked).tobytes(), (name, s, got[0][s])
    plain = _plain_sums(c, c['raw'])
    one = _device_strata(monkeypatch, poison, c, (), None, launches=1)
    assert one.shape == (1, 1, 10) and one[0][0].tobytes() == plain.tobytes(), 'no edges, no ground plane: the row of depth_metric_sums'
    assert np.array_equal(got[0][:, :4].sum(0), plain[:4]), 'n and the three counts add up over the strata'
    assert {s for s in range(c['S']) if got[0][s, 0] > 0} == c['populated'] and not got[0][sorted(c['empty'])].any()


@pytest.mark.parametrize('name', list(SC.CASES))
def test_rows_vs_float64(monkeypatch, name):
    c = SC.CASES[name]
    got = _device_strata(monkeypatch, memguard.POISONS[0], c, c['edges'], c['ground'], launches=1)[0]
    ref = SR.strata_sums(c['raw'], c['pred'], c['ground'], c['geom'], c['rect'], c['edges'], c['tol'])
    for s in range(c['S']):
        TE._assert_sums(got[s], ref[s], f'{name} stratum {s}')


# ------------------------------------------------------------------------------------------------ the batch entry point
BATCH_GEOMS = ((9, 28, 1, 4, 8, 24), (11, 27, 3, 3, 8, 24), (13, 36, 5, 8, 8, 24))       # vector loads, scalar loads, vector loads


def _batch_frames():
    """Three (geom, raw, pred, ground) of different sizes and offsets; the second frame's plane is invalid everywhere (-5: nothing on the
    ground there)."""
    out = []
    for k, geom in enumerate(BATCH_GEOMS):
        raw, pred = TE._inputs(geom, 50 + k)
        ground = SC._ground(geom, raw, 50 + k)
        if k == 1:
            ground[...] = -5.0
        out.append((geom, raw, pred, ground))
    return out


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('with_ground', [True, False], ids=['ground', 'bins-only'])
def test_batch_blocks_carry_the_bits_of_the_single_image_entry_point(monkeypatch, with_ground, poison):
    from gedepth_amd import hip
    from gedepth_amd import kernels as K
    frames = _batch_frames()
    n, (Hc, Wc), rect = len(frames), (8, 24), (1, 8, 2, 23)
    S = SR.count(SC.EDGES, True if with_ground else None)
    pred = torch.from_numpy(np.stack([f[2] for f in frames])).cuda()
    ref = torch.zeros(n, S, 10, device='cuda', dtype=torch.float64)
    for f, (geom, raw, _, ground) in enumerate(frames):
        K.depth_metric_sums_strata(pred[f], torch.from_numpy(raw).cuda(), geom[2], geom[3], rect, *LIMITS, ref[f], SC.EDGES,
                                   torch.from_numpy(ground).cuda() if with_ground else None, SC.TOL)
    guard = _install(monkeypatch, poison)
    d_pred = guard.framed(pred)
    gts = [guard.framed(torch.from_numpy(f[1]).cuda()) for f in frames]
    grounds = [guard.framed(torch.from_numpy(f[3]).cuda()) for f in frames] if with_ground else None
    rows = guard.proxy.empty(n + 2, S, 10, device='cuda', dtype=torch.float64)
    tops, lefts = [f[0][2] for f in frames], [f[0][3] for f in frames]
    K.depth_metric_sums_strata_batch(d_pred, gts, tops, lefts, rect, *LIMITS, rows, SC.EDGES, grounds, SC.TOL)
    K.depth_metric_sums_strata_batch(d_pred, gts[:1], tops[:1], lefts[:1], rect, *LIMITS, rows[n + 1:], SC.EDGES, grounds and grounds[:1], SC.TOL)
    torch.cuda.synchronize()
    monkeypatch.undo()
    checked = guard.check()                                           # red zones of pred, the ground truths, the planes, the partials and the sums
    assert guard.launched == ['ge_depth_metrics_strata_batch'] * 2 and 'ge_depth_metrics_strata_workspace' in guard.direct
    ws = [f for f in checked if os.path.basename(f.site[0]) == 'strata_kernels.py']
    assert len(ws) == 1 and ws[0].nbytes == hip.lib().ge_depth_metrics_strata_workspace(8, Hc, Wc, S)
    stay = memguard.poisoned(rows, poison).cpu().numpy()
    assert stay[n].all() and not stay[:n].any() and not stay[n + 1].any(), 'the block after the last image must stay poisoned'
    got = rows.cpu().numpy()
    want = ref.cpu().numpy()
    assert got[:n].tobytes() == want.tobytes(), (got[:n], want)
    assert got[n + 1].tobytes() == want[0].tobytes()
    for f, (geom, raw, p, ground) in enumerate(frames):               # the independent reference
        f64 = SR.strata_sums(raw, p, ground if with_ground else None, geom, rect, SC.EDGES, SC.TOL)
        for s in range(S):
            TE._assert_sums(got[f][s], f64[s], f'batch image {f} stratum {s}')
    if with_ground:
        assert got[0][1::2, 0].sum() > 0 and got[2][1::2, 0].sum() > 0 and got[1][1::2, 0].sum() == 0      # the invalid plane: nothing on the ground
        assert got[1][0::2, 0].sum() > 0


def test_wrapper_errors_on_the_device():
    from gedepth_amd import kernels
    pred, raw = torch.zeros(8, 20, device='cuda'), torch.zeros(11, 27, device='cuda', dtype=torch.uint16)
    out = torch.zeros(4, 10, device='cuda', dtype=torch.float64)
    with pytest.raises(RuntimeError, match='bad argument'):
        kernels.depth_metric_sums_strata(pred, raw, 4, 3, (0, 8, 0, 20), *LIMITS, out, SC.EDGES)           # the window leaves the frame
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums_strata(pred, raw, 3, 3, (0, 8, 0, 20), *LIMITS, out[:2], (), torch.zeros(11, 27))


# ------------------------------------------------------------------------------------------------ the loop, on the toy tree
def _ground_following_tree(root):
    """``make_toy_kitti``'s tree with every ground-truth PNG overwritten: the same 5 % of returns, but below the horizon row about half of
    them lie on the plane of pe_165.npy times uniform(0.95, 1.05)."""
    split = make_toy_kitti(root, seed=3)
    plane = np.load(os.path.join(root, 'input', '2011_09_26', 'pe', 'pe_165.npy'))
    rng = np.random.default_rng(77)
    H, W = plane.shape
    for folder, _, files in sorted(os.walk(os.path.join(root, 'gt_depth'))):
        for name in sorted(f for f in files if f.endswith('.png')):
            depth = np.where(rng.random((H, W)) < 0.05, rng.uniform(1.0, 80.0, (H, W)), 0.0)
            on = (depth > 0) & (plane > 0) & (rng.random((H, W)) < 0.5)
            depth = np.where(on, plane * rng.uniform(0.95, 1.05, (H, W)), depth)
            Image.fromarray(np.minimum(depth * 256, 65535).astype(np.uint16)).save(os.path.join(folder, name))
    return split, plane.astype(np.float32)


def _reference_counts(ds, plane, spec):
    """(N, S) pixel counts of every split entry from its PNG and the plane, through tests/strata_ref.py."""
    out = []
    for i in range(len(ds)):
        raw = ds.gt_raw(i)
        h, w = raw.shape
        geom = (h, w, h - 352, int((w - 1216) / 2), 352, 1216)
        _, _, stratum = SR.window_strata(raw, plane if spec.ground else None, geom, ds.eval_rect(352, 1216), spec.edges, spec.ground_tol,
                                         (ds.depth_scale, ds.min_depth, ds.max_depth))
        out.append([int((stratum == s).sum()) for s in range(spec.count)])
    return np.array(out)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    from gedepth_amd.depth.core import StrataSpec
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    import test_inference_gpu as TI
    root = str(tmp_path_factory.mktemp('kitti_strata'))
    split, plane = _ground_following_tree(root)
    model = TI._model('depthformer_swint_v.py', root, split)
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    counts = _reference_counts(ds, plane, StrataSpec())               # host only: what the tree must hold before the GPU is asked
    both = [(counts[:, 2 * b] > 0).all() and (counts[:, 2 * b + 1] > 0).all() for b in range(4)]
    assert sum(both) >= 3, counts
    return model, ds, plane, counts, (lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False))


def _plain_loop_on_the_same_maps(monkeypatch, ds):
    """Two runs of the forward differ in the last bits (float atomics; tests/test_inference_gpu.py bounds it), so the list of a second call
    cannot be compared with ``==``.  Instead every map the strata loop reduces also goes, on the same stream and before the strata call,
    through the very call the loop makes without ``strata`` (``pre_eval_device`` / ``pre_eval_device_batch`` with the same arguments) into
    a buffer of this test: ``tuples()`` is the list the loop without ``strata`` returns for these maps."""
    from gedepth_amd.depth.core import metrics_from_sums
    sums = torch.zeros(len(ds), 10, device='cuda', dtype=torch.float64)
    seen = []
    single, batch = ds.pre_eval_device_strata, ds.pre_eval_device_strata_batch

    def spy_single(pred, index, rows, spec, ground, **kw):
        ds.pre_eval_device(pred, index, sums[len(seen)])
        seen.append(index)
        return single(pred, index, rows, spec, ground, **kw)

    def spy_batch(preds, indices, rows, spec, grounds, raws=None, **kw):
        ds.pre_eval_device_batch(preds, indices, sums[len(seen):len(seen) + len(indices)], raws=raws)
        seen.extend(indices)
        return batch(preds, indices, rows, spec, grounds, raws=raws, **kw)
    monkeypatch.setattr(ds, 'pre_eval_device_strata', spy_single, raising=False)
    monkeypatch.setattr(ds, 'pre_eval_device_strata_batch', spy_batch, raising=False)
    return seen, lambda: [metrics_from_sums(r) for r in sums.cpu().numpy()]


def test_loop_returns_the_plain_results_and_exact_counts(toy, monkeypatch):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core import StrataSpec
    model, ds, plane, counts, loader = toy
    spec = StrataSpec()
    for F in (1, 2):
        seen, tuples = _plain_loop_on_the_same_maps(monkeypatch, ds)
        results, rows = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, eval_batch=F, strata=spec)
        monkeypatch.undo()
        plain = tuples()
        assert seen == list(range(len(ds))) and results == plain, (F, results, plain)
        assert isinstance(rows, np.ndarray) and rows.shape == (len(ds), spec.count, 10) and rows.dtype == np.float64
        assert np.array_equal(rows[..., 0], counts), (F, rows[..., 0], counts)
        for i, t in enumerate(results):
            n = rows[i, :, 0].sum()
            assert n == int(ds.eval_mask(ds.eval_kb_crop(ds._gt(i))).sum()) > 1000
            assert all(abs(t[k] * n - round(t[k] * n)) < 1e-6 for k in range(3))                 # the n behind the tuple
            assert np.array_equal(rows[i, :, 1:4].sum(0), [round(t[k] * n) for k in range(3)])
        flat = ds.evaluate_strata(rows, spec)
        assert len(flat) == spec.count * 11 and all(np.isfinite(v) or np.isnan(v) for v in flat.values())
        assert sum(v for k, v in flat.items() if k.endswith('.pixels')) == pytest.approx(1.0, abs=1e-12)
