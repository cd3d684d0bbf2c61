"""Device evaluation on the MI355X: ``ge_depth_metrics`` (csrc/eval.hip) against a float64 numpy restatement under red zones and poison
(tests/memguard.py), the device metric tuple against the float32 host ``metrics``, and ``single_gpu_test(device_eval=True)`` against the
host loop on the toy KITTI tree.

Bounds.  The counts (n and the three thresholds) are integers and must be equal.  The continuous sums are compared with tests/eval_ref.py:
1e-12 relative, 1e-9 for the three sums that hold a device ``log`` / ``log10``.  The device tuple is compared with the host's float32
``metrics`` through the host's own float32 error: ``gap`` = |metrics - float64 restatement|, measured on the CPU on the inputs of each
comparison, and the bound is 2 * gap + 1e-9.  Measured gaps on these inputs (numpy 2.2, float32 pairwise sums), largest over the kernel
cases: abs_rel 3.9e-08, rmse 1.2e-06, log_10 1.1e-07, rmse_log 3.6e-08, silog 6.8e-06, sq_rel 7.6e-07 (a1 .. a3: 0)."""
import os

import numpy as np
import pytest
import torch

import eval_ref as R
import memguard
from toy_kitti import make_toy_kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
pytestmark = pytest.mark.gpu

LIMITS = (256, 1e-3, 80)                                      # depth_scale, min_depth, max_depth
ENGINE_EPS = 2e-4             # engine vs aug_test, per pixel and relative: the bound test_inference_gpu.py asserts (`mx <= 2e-4`)


def _full(g):
    return (0, g[4], 0, g[5])


def _inputs(geom, seed, gt='mixed'):
    """(raw uint16 (H, W), pred f32 (Hc, Wc)): a quarter of the pixels without a return, a tenth at or beyond max_depth (20480 / 256 is
    exactly 80, which is not < 80), the rest 1 .. 79.7 m; predictions within a factor 2 of the ground truth where there is one."""
    H, W, top, left, Hc, Wc = geom
    rng = np.random.default_rng(seed)
    raw = rng.integers(257, 20400, (H, W)).astype(np.uint16)
    u = rng.random((H, W))
    raw[u < 0.25] = 0
    far = (u >= 0.25) & (u < 0.35)
    raw[far] = rng.integers(20480, 65536, int(far.sum())).astype(np.uint16)
    if H * W == 1:
        raw[...] = 2560
    if gt == 'zero':
        raw[...] = 0
    elif gt == 'far':
        raw = rng.integers(20480, 65536, (H, W)).astype(np.uint16)
    g = R.window(raw, top, left, Hc, Wc)
    pred = np.where((g > 0) & (g < 80), g * rng.uniform(0.5, 2.0, (Hc, Wc)), rng.uniform(1.0, 80.0, (Hc, Wc))).astype(np.float32)
    return raw, pred


def _threshold_inputs(left):
    """336 pixels whose ratio lies within a few float32 ulps of 1.25, 1.25^2 or 1.25^3, on both sides and on both branches of the
    maximum (gt / pred and pred / gt), as a (12, 28) crop of a (13, 32 - (left & 1)) frame."""
    raws, preds = [], []
    for raw in [256 * k for k in (1, 3, 10, 37, 79)] + [1234, 4321, 19999]:
        g = np.float32(raw) / np.float32(256)
        for p in (1, 2, 3):
            t = np.float32(1.25 ** p)
            for base in (g / t, g * t):
                lo = hi = np.float32(base)
                cands = [lo]
                for _ in range(3):
                    lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
                    cands += [lo, hi]
                raws += [raw] * len(cands)
                preds += cands
    geom = (13, 32 - (left & 1), 1, left, 12, 28)
    raw = np.zeros(geom[:2], np.uint16)
    raw[1:13, left:left + 28] = np.array(raws, np.uint16).reshape(12, 28)
    return geom, raw, np.array(preds, np.float32).reshape(12, 28)


def _nan_zero_inputs():
    geom = (9, 28, 1, 4, 8, 24)
    raw, pred = _inputs(geom, 7)
    raw[1 + 2, 4 + 5] = raw[1 + 6, 4 + 17] = 2560                    # both pixels count
    pred[2, 5], pred[6, 17] = np.nan, 0.0
    return geom, raw, pred


def _cases():
    out = {}
    for name, geom in (('odd-left-scalar-gt', (11, 27, 3, 3, 8, 20)), ('vector', (9, 28, 1, 4, 8, 24)), ('one-pixel', (1, 1, 0, 0, 1, 1)),
                       ('multi-block-tails', (40, 530, 2, 9, 37, 515))):
        out[name] = (geom,) + _inputs(geom, len(out)) + (_full(geom),)
    big = (40, 530, 2, 9, 37, 515)
    out['garg-rect'] = (big,) + _inputs(big, 11) + ((int(0.40810811 * 37), int(0.99189189 * 37), int(0.03594771 * 515), int(0.96405229 * 515)),)
    out['empty-rows'] = (big,) + _inputs(big, 12) + ((5, 5, 0, 515),)
    out['empty-cols'] = (big,) + _inputs(big, 12) + ((0, 37, 7, 7),)
    out['gt-all-zero'] = (big,) + _inputs(big, 13, 'zero') + (_full(big),)
    out['gt-all-beyond-max'] = (big,) + _inputs(big, 14, 'far') + (_full(big),)
    for left in (4, 3):
        geom, raw, pred = _threshold_inputs(left)
        out[f'thresholds-left{left}'] = (geom, raw, pred, _full(geom))
    geom, raw, pred = _nan_zero_inputs()
    out['nan-and-zero-pred'] = (geom, raw, pred, _full(geom))
    return out


CASES = _cases()


def _host(case):
    """(gt, pred) of the pixels that count, as 1-D float32 arrays: what ``pre_eval`` hands to ``metrics``."""
    geom, raw, pred, rect = CASES[case] if isinstance(case, str) else case
    g = R.window(raw, *geom[2:], depth_scale=LIMITS[0])
    m = R.mask_of(g, rect, LIMITS[1], LIMITS[2])
    return g[m], pred[m]


def _device_sums(monkeypatch, poison, geom, raw, pred, rect, launches=1):
    """``launches`` runs of kernels.depth_metric_sums into rows 1.. of a framed (launches + 2, 10) buffer, inputs and workspace framed too."""
    from gedepth_amd import eval_kernels, hip, kernels
    guard = memguard.Guard(poison)
    monkeypatch.setattr(eval_kernels, '_WS', {})                      # a workspace cached by an earlier test would bypass the frames
    guard.install(monkeypatch, [eval_kernels], binding=hip)
    d_pred, d_raw = guard.framed(torch.from_numpy(pred).cuda()), guard.framed(torch.from_numpy(raw).cuda())
    sums = guard.proxy.empty(launches + 2, 10, device='cuda', dtype=torch.float64)
    for k in range(launches):
        kernels.depth_metric_sums(d_pred, d_raw, geom[2], geom[3], rect, *LIMITS, sums[1 + k])
    torch.cuda.synchronize()
    monkeypatch.undo()
    frames = guard.check()                                            # red zones of pred, gt_raw, partials and sums
    assert guard.launched == ['ge_depth_metrics'] * launches and 'ge_depth_metrics_workspace' in guard.direct
    ws = [f for f in frames if os.path.basename(f.site[0]) == 'eval_kernels.py']
    assert len(ws) == 1 and ws[0].nbytes == hip.lib().ge_depth_metrics_workspace(geom[4], geom[5]) and not bool(ws[0].poisoned().any())
    stay = memguard.poisoned(sums, poison).cpu().numpy()
    assert stay[0].all() and stay[-1].all() and not stay[1:-1].any(), 'rows next to the written ones must stay poisoned'
    return sums.cpu().numpy()[1:-1]


def _assert_sums(got, ref, what):
    assert np.array_equal(got[:4], ref[:4]), (what, got[:4], ref[:4])               # n and the three counts: integers
    for k in range(4, 10):
        tol = 1e-9 if k in R.LOG_SUMS else 1e-12
        if np.isfinite(ref[k]):
            print(f'[{what}] {R.SUM_NAMES[k]}: device {got[k]!r} f64 {ref[k]!r} rel {abs(got[k] - ref[k]) / max(abs(ref[k]), 1e-300):.1e}')
            assert abs(got[k] - ref[k]) <= tol * abs(ref[k]), (what, R.SUM_NAMES[k], got[k], ref[k])
        else:
            assert (np.isnan(ref[k]) and np.isnan(got[k])) or got[k] == ref[k], (what, R.SUM_NAMES[k], got[k], ref[k])


def _assert_tuple(dev, gt, pred, what, extra=None):
    """The device tuple against the host's float32 ``metrics``: counts through a * n, the rest within 2 * gap + 1e-9 (+ ``extra[name]``)."""
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES, metrics
    with np.errstate(all='ignore'):
        host = metrics(gt, pred, LIMITS[1], LIMITS[2])
    f64 = R.calculate_f64(gt, pred)
    n = gt.size
    if n == 0:
        assert all(np.isnan(v) for v in dev) and all(np.isnan(v) for v in host)
        return
    for k, name in enumerate(METRIC_NAMES):
        if k < 3:
            if extra is None:
                assert round(dev[k] * n) == round(host[k] * n), (what, name, dev[k] * n, host[k] * n)
        elif not np.isfinite(host[k]) or not np.isfinite(f64[k]):
            assert np.isnan(dev[k]) == np.isnan(host[k]), (what, name, dev[k], host[k])
        else:
            gap = abs(host[k] - f64[k])
            bound = 2 * gap + 1e-9 + (extra[name] if extra else 0.0)
            print(f'[{what}] {name}: device {dev[k]!r} host {host[k]!r} gap {gap:.1e} bound {bound:.1e}')
            assert abs(dev[k] - host[k]) <= bound, (what, name, dev[k], host[k], bound)


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('case', list(CASES))
def test_metric_sums_vs_float64_under_guards(monkeypatch, case, poison):
    from gedepth_amd.depth.core import metrics_from_sums
    geom, raw, pred, rect = CASES[case]
    gt_m, pred_m = _host(case)
    got = _device_sums(monkeypatch, poison, geom, raw, pred, rect, launches=2)
    assert got[0].tobytes() == got[1].tobytes(), 'two launches on the same input must give the same bits'
    _assert_sums(got[0], R.sums_f64(gt_m, pred_m), case)
    _assert_tuple(metrics_from_sums(got[0]), gt_m, pred_m, case)
    if case.startswith(('empty', 'gt-all')):
        assert gt_m.size == 0 and got[0][0] == 0 and not got[0].any()
    else:
        assert gt_m.size > 0


def test_threshold_inputs_straddle_every_threshold():
    """The property the threshold cases rely on (host only): for each threshold there are ratios within one float32 ulp below and at / above it."""
    gt, pred = _host('thresholds-left4')
    ratio = np.maximum(gt / pred, pred / gt)
    for p in (1, 2, 3):
        t = np.float32(1.25 ** p)
        ulp = np.spacing(t)
        assert ((ratio < t) & (ratio >= t - ulp)).any() and ((ratio >= t) & (ratio <= t + ulp)).any(), p
        assert (ratio == t).any(), p


def test_wrapper_argument_errors():
    from gedepth_amd import kernels
    pred, raw = torch.zeros(8, 20, device='cuda'), torch.zeros(11, 27, device='cuda', dtype=torch.uint16)
    out = torch.zeros(10, device='cuda', dtype=torch.float64)
    with pytest.raises(RuntimeError, match='bad argument'):
        kernels.depth_metric_sums(pred, raw, 4, 3, (0, 8, 0, 20), *LIMITS, out)           # the window leaves the frame
    with pytest.raises(RuntimeError, match='bad argument'):
        kernels.depth_metric_sums(pred, raw, 3, 3, (0, 9, 0, 20), *LIMITS, out)           # the rectangle leaves the crop
    with pytest.raises(TypeError):
        kernels.depth_metric_sums(pred.double(), raw, 3, 3, (0, 8, 0, 20), *LIMITS, out)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums(pred, raw.cpu(), 3, 3, (0, 8, 0, 20), *LIMITS, out)


# ------------------------------------------------------------------------------------------------ the loop, on the toy tree
def _engine_extra(gt, pred, eps=ENGINE_EPS):
    """How far each continuous metric can move when every prediction moves by at most ``eps`` relative (|dq| <= eps q, |d log q| <= le):
    abs_rel <= mean(dq / g); sq_rel <= mean((2 |d| dq + dq^2) / g); rmse, rmse_log and silog / 100 are norms (of d, l and l - mean l), so
    they move by at most the norm of the change: sqrt(mean dq^2), le and le; log_10 <= le / ln 10."""
    g, q = gt.astype(np.float64), pred.astype(np.float64)
    dq, d, le = eps * q, np.abs(g - q), -np.log1p(-eps)
    return dict(abs_rel=np.mean(dq / g), sq_rel=np.mean((2 * d * dq + dq * dq) / g), rmse=np.sqrt(np.mean(dq * dq)), log_10=le / np.log(10),
                rmse_log=le, silog=100 * le)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import test_inference_gpu as TI
    root = str(tmp_path_factory.mktemp('kitti_device_eval'))
    split = make_toy_kitti(root, seed=3)
    model = TI._model('depthformer_swint_v.py', root, split)
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    return model, ds, (lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False))


def _counted(ds, i, pred_map):
    gt = ds.eval_kb_crop(ds._gt(i))
    mask = ds.eval_mask(gt)
    return gt[mask], pred_map[mask]


def test_pre_eval_device_on_the_maps_of_aug_test(toy):
    """``pre_eval_device`` fed with the very maps ``aug_test`` returned: the engine is out of this comparison, so the counts must be equal."""
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core import metrics_from_sums
    model, ds, loader = toy
    maps = single_gpu_test(model, loader())
    assert len(maps) == len(ds) == 4 and all(m.shape == (1, 352, 1216) and m.dtype == np.float32 for m in maps)
    sums = torch.full((len(maps) + 1, 10), -7.0, device='cuda', dtype=torch.float64)
    for i, m in enumerate(maps):
        ds.pre_eval_device(torch.from_numpy(m).cuda(), i, sums[i])
    rows = sums.cpu().numpy()
    assert (rows[-1] == -7.0).all()
    for i, m in enumerate(maps):
        gt_m, pred_m = _counted(ds, i, m)
        host = ds.pre_eval([m], [i])[0][0]
        dev = metrics_from_sums(rows[i])
        assert rows[i][0] == gt_m.size > 1000
        assert [round(host[k] * gt_m.size) for k in range(3)] == list(rows[i][1:4])
        _assert_sums(rows[i], R.sums_f64(gt_m, pred_m), f'frame {i}')
        _assert_tuple(dev, gt_m, pred_m, f'frame {i}')
    with pytest.raises(TypeError):
        ds.pre_eval_device(torch.from_numpy(maps[0]), 0, sums[0])                        # a host map


def test_device_eval_loop_vs_host_loop(toy):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    model, ds, loader = toy
    maps = single_gpu_test(model, loader())
    host = single_gpu_test(model, loader(), pre_eval=True)
    model.__dict__.pop('_ge_inferencers', None)
    dev = single_gpu_test(model, loader(), pre_eval=True, device_eval=True)
    eng = model._ge_inferencers[False]
    assert eng.captures == 1 and len(dev) == len(host) == 4                              # two eager frames, the capture, a replay
    assert all(isinstance(t, tuple) and len(t) == 9 for t in dev)
    for i, (d, h) in enumerate(zip(dev, host)):
        gt_m, pred_m = _counted(ds, i, maps[i])
        n = gt_m.size
        ratio = np.maximum(gt_m / pred_m, pred_m / gt_m)
        for k in range(3):                           # a count moves by at most the pixels whose ratio the engine's bound can carry across
            near = int((np.abs(ratio - 1.25 ** (k + 1)) <= 1.25 ** (k + 1) * 2 * ENGINE_EPS).sum())
            print(f'[loop frame {i}] {METRIC_NAMES[k]}: device {d[k] * n:.0f} host {h[k] * n:.0f} of {n}, {near} pixels near the threshold')
            assert abs(round(d[k] * n) - round(h[k] * n)) <= near, (i, METRIC_NAMES[k], d[k] * n, h[k] * n, near)
            assert abs(d[k] * n - round(d[k] * n)) < 1e-6                                # same n on both sides
        _assert_tuple(d, gt_m, pred_m, f'loop frame {i}', extra=_engine_extra(gt_m, pred_m))
    summary = ds.evaluate(dev)                                                           # the list works where pre_eval's does
    assert set(summary) == set(METRIC_NAMES) and all(np.isfinite(v) for v in summary.values())


def test_device_eval_refuses_what_it_cannot_do(toy):
    from gedepth_amd.depth.apis.test import multi_gpu_test, single_gpu_test
    from gedepth_amd.depth.datasets.ddad import DDADDataset
    model, ds, loader = toy
    with pytest.raises(NotImplementedError, match='show'):
        single_gpu_test(model, loader(), pre_eval=True, device_eval=True, show=True)
    with pytest.raises(NotImplementedError, match='show'):
        multi_gpu_test(model, loader(), pre_eval=True, device_eval=True, out_dir='/nonexistent')
    with pytest.raises(NotImplementedError, match='pre_eval'):
        single_gpu_test(model, loader(), device_eval=True)

    class DDADLoader:
        dataset = DDADDataset.__new__(DDADDataset)
        batch_sampler = [[0]]
    with pytest.raises(NotImplementedError, match='DDADDataset'):
        single_gpu_test(model, DDADLoader(), pre_eval=True, device_eval=True)
    cfg = model.cfg
    try:
        model.cfg = None
        with pytest.raises(NotImplementedError, match='model.cfg'):
            single_gpu_test(model, loader(), pre_eval=True, device_eval=True)
    finally:
        model.cfg = cfg


def test_engine_to_host_false_returns_the_device_buffer(toy):
    from gedepth_amd.depth.apis.inference import DepthInferencer
    model, ds, _ = toy
    path = os.path.join(ds.img_dir, ds.img_infos[0]['filename'])
    eng = DepthInferencer(model)
    t = eng(path, graph=False, to_host=False)
    assert t is eng.static_out and t.is_cuda and t.shape == (1, 352, 1216) and t.dtype == torch.float32
    kept = t.clone()                                               # on the current stream, which waits for the engine's
    host = eng(path, graph=False)                                  # to_host=True, the default
    assert isinstance(host, np.ndarray) and host.shape == (1, 352, 1216)
    assert np.array_equal(eng.static_out.cpu().numpy(), host)      # the array is the buffer's content
    a = kept.cpu().numpy()
    # two runs of the forward are not bit-reproducible (float atomics): the bound of test_inference_gpu.py::test_graph_replay
    print(f'\n[to_host] bit-identical across two calls: {np.array_equal(a, host)}')
    assert np.abs(a - host).max() <= 1e-6 * np.abs(host).max()
