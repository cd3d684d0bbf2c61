"""The DDAD test protocol on the MI355X: ``ge_depth_metrics_resized`` (csrc/eval.hip) and ``ge_infer_front_ddad`` (csrc/infer.hip) under red
zones and poison (tests/memguard.py), the DDAD branch of ``DepthInferencer`` and ``single_gpu_test(device_eval=True)`` on the toy DDAD tree.

Two references (tests/ddad_ref.py).  The float32 RESTATEMENT of the kernel's resampling: the counts (n and the three thresholds) must be
equal, the continuous sums agree with ``eval_ref.sums_f64`` on the restated predictions to 1e-12 relative, 1e-9 for the three sums that hold
a device ``log`` / ``log10``.  The HOST path (``DDADDataset.pre_eval``: ATen's ``F.interpolate``) differs from the kernel by at most
``HOST_BAND`` = 1e-6 relative per pixel (measured 2.7e-7 on these geometries, tests/test_ddad_device_cpu.py): n must be equal, a threshold
count may differ by the number of counted pixels whose host ratio lies within that band of the threshold, and a continuous metric by
2 * gap + 1e-9 + extra, with ``gap`` the host's own float32 error against float64 and ``extra`` how far the metric can move when every
prediction moves by the band (``_engine_extra``).  Loop comparisons add ``ENGINE_EPS``, the engine-versus-``simple_test`` bound."""
import contextlib
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import ddad_ref as D
import eval_ref as R
import memguard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
pytestmark = pytest.mark.gpu

LIMITS = (1e-3, 200)                                          # min_depth, max_depth of the DDAD configs
ENGINE_EPS = 2e-4            # engine vs simple_test, per pixel and relative (measured 3.3e-6): test_engine_eager_vs_simple_test asserts it
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


# ------------------------------------------------------------------------------------------------ the metric kernel
def _gt(H, W, seed, kind='sparse'):
    """'sparse': about 10 % of the pixels valid in 1 .. 150 m, 3 % at exactly max_depth (200.0 is not < 200), 3 % beyond, the rest 0."""
    rng = np.random.default_rng(seed)
    if kind == 'zero':
        return np.zeros((H, W), np.float32)
    if kind == 'dense':
        return rng.uniform(1, 150, (H, W)).astype(np.float32)
    u = rng.random((H, W))
    gt = np.where(u < 0.10, rng.uniform(1, 150, (H, W)), 0.0)
    gt[(u >= 0.10) & (u < 0.13)] = 200.0
    gt[(u >= 0.13) & (u < 0.16)] = 230.5
    gt.flat[0] = 10.0                                          # the small geometries count at least one pixel
    return gt.astype(np.float32)


def _pred(h, w, seed):
    return np.random.default_rng(1000 + seed).uniform(1, 150, (h, w)).astype(np.float32)


def _threshold_inputs():
    """Identity geometry (12, 28): 336 pixels whose ratio lies within a few float32 ulps of 1.25, 1.25^2 or 1.25^3, on both sides and on
    both branches of the maximum (the idea of test_eval_device_gpu.py::_threshold_inputs)."""
    gts, preds = [], []
    for g in (1.0, 3.0, 10.0, 37.0, 79.0, 4.8203125, 16.87890625, 148.25):
        g = np.float32(g)
        for p in (1, 2, 3):
            t = np.float32(1.25 ** p)
            for base in (g / t, g * t):
                lo = hi = np.float32(base)
                cands = [lo]
                for _ in range(3):
                    lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
                    cands += [lo, hi]
                gts += [g] * len(cands)
                preds += cands
    return np.array(preds, np.float32).reshape(12, 28), np.array(gts, np.float32).reshape(12, 28)


def _cases():
    out = {}
    for k, ((h, w), (H, W)) in enumerate(D.GEOMETRIES):
        out[f'{h}x{w}-{H}x{W}'] = (_pred(h, w, k), _gt(H, W, k))
    out['gt-all-zero'] = (_pred(48, 80, 20), _gt(200, 532, 20, 'zero'))
    out['dense-vector'] = (_pred(12, 20, 21), _gt(36, 64, 21, 'dense'))
    out['dense-scalar'] = (_pred(12, 20, 22), _gt(37, 61, 22, 'dense'))
    out['thresholds'] = _threshold_inputs()
    # a NaN tap makes every pixel it enters NaN, with weight 0 too (0 * NaN), in the kernel as in ATen; not on an identity geometry, where
    # ATen copies the map instead of interpolating it
    pred, gt = _pred(8, 12, 23), _gt(20, 31, 23, 'dense')
    pred[2, 5], pred[6, 7] = np.nan, 0.0
    out['nan-and-zero-pred'] = (pred, gt)
    return out


CASES = _cases()


def _counted(pred, gt, resize):
    """(gt, resized prediction) of the pixels that count, as 1-D float32 arrays."""
    m = D.mask_of(gt, *LIMITS)
    return gt[m], resize(pred, *gt.shape)[m]


def _device_sums(monkeypatch, poison, pred, gt, launches=1):
    """``launches`` runs of kernels.depth_metric_sums_resized into rows 1.. of a framed (launches + 2, 10) buffer, inputs and workspace framed."""
    from gedepth_amd import eval_kernels, hip, kernels
    guard = memguard.Guard(poison)
    monkeypatch.setattr(eval_kernels, '_WS', {})
    guard.install(monkeypatch, [eval_kernels], binding=hip)
    d_pred, d_gt = guard.framed(torch.from_numpy(pred).cuda()), guard.framed(torch.from_numpy(gt).cuda())
    sums = guard.proxy.empty(launches + 2, 10, device='cuda', dtype=torch.float64)
    for k in range(launches):
        kernels.depth_metric_sums_resized(d_pred, d_gt, *LIMITS, sums[1 + k])
    torch.cuda.synchronize()
    monkeypatch.undo()
    frames = guard.check()                                            # red zones of pred, gt, partials and sums
    assert guard.launched == ['ge_depth_metrics_resized'] * launches and 'ge_depth_metrics_resized_workspace' in guard.direct
    ws = [f for f in frames if os.path.basename(f.site[0]) == 'eval_kernels.py']
    assert len(ws) == 1 and ws[0].nbytes == hip.lib().ge_depth_metrics_resized_workspace(*gt.shape) and not bool(ws[0].poisoned().any())
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


def _engine_extra(gt, pred, eps):
    """test_eval_device_gpu.py::_engine_extra: how far each continuous metric can move when every prediction moves by at most ``eps``
    relative."""
    g, q = gt.astype(np.float64), pred.astype(np.float64)
    dq, d, le = eps * q, np.abs(g - q), -np.log1p(-eps)
    return dict(abs_rel=np.mean(dq / g), sq_rel=np.mean((2 * d * dq + dq * dq) / g), rmse=np.sqrt(np.mean(dq * dq)), log_10=le / np.log(10),
                rmse_log=le, silog=100 * le)


def _assert_vs_host(dev, gt, pred, what, eps, band=None):
    """The device tuple ``dev`` against the host's float32 ``metrics`` on (gt, pred) = the counted pixels with ATen's resized predictions:
    equal n is the caller's; a count within the pixels whose host ratio lies within ``band`` (relative; ``eps`` itself unless given) of
    its threshold; the rest within 2 * gap + 1e-9 + extra(eps)."""
    band = eps if band is None else band
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES, metrics
    n = gt.size
    if n == 0:
        assert all(np.isnan(v) for v in dev)
        return
    with np.errstate(all='ignore'):
        host = metrics(gt, pred, *LIMITS)
    f64 = R.calculate_f64(gt, pred)
    extra = _engine_extra(gt, pred, eps)
    for k, name in enumerate(METRIC_NAMES):
        if k < 3:
            near = D.near_threshold(gt, pred, k + 1, band)
            print(f'[{what}] {name}: device {dev[k] * n:.0f} host {host[k] * n:.0f} of {n}, {near} pixels near the threshold')
            assert abs(round(dev[k] * n) - round(host[k] * n)) <= near, (what, name, dev[k] * n, host[k] * n, near)
            assert abs(dev[k] * n - round(dev[k] * n)) < 1e-6                                # same n on both sides
        elif not np.isfinite(host[k]) or not np.isfinite(f64[k]):
            assert np.isnan(dev[k]) == np.isnan(host[k]), (what, name, dev[k], host[k])
        else:
            gap = abs(host[k] - f64[k])
            bound = 2 * gap + 1e-9 + extra[name]
            print(f'[{what}] {name}: device {dev[k]!r} host {host[k]!r} gap {gap:.1e} bound {bound:.1e}')
            assert abs(dev[k] - host[k]) <= bound, (what, name, dev[k], host[k], bound)


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('case', list(CASES))
def test_resized_metric_sums_under_guards(monkeypatch, case, poison):
    from gedepth_amd.depth.core import metrics_from_sums
    pred, gt = CASES[case]
    got = _device_sums(monkeypatch, poison, pred, gt, launches=2)
    assert got[0].tobytes() == got[1].tobytes(), 'two launches on the same input must give the same bits'
    gt_m, pred_m = _counted(pred, gt, D.resize_f32)
    _assert_sums(got[0], R.sums_f64(gt_m, pred_m), case)
    gt_h, pred_h = _counted(pred, gt, D.resize_host)
    assert got[0][0] == gt_h.size                                                    # the mask depends on the ground truth only
    _assert_vs_host(metrics_from_sums(got[0]), gt_h, pred_h, case, D.HOST_BAND)
    if case == 'gt-all-zero':
        assert gt_m.size == 0 and not got[0].any()
    else:
        assert gt_m.size > 0
    if case == '8x12-8x12':                                                          # identity: every w1 == 0, the taps are the pixels
        m = D.mask_of(gt, *LIMITS)
        _assert_sums(got[0], R.sums_f64(gt[m], pred[m]), case + ' (pred itself)')


def test_threshold_inputs_straddle_every_threshold():
    pred, gt = CASES['thresholds']
    with np.errstate(all='ignore'):
        ratio = np.maximum(gt / pred, pred / gt).ravel()
    for p in (1, 2, 3):
        t = np.float32(1.25 ** p)
        ulp = np.spacing(t)
        assert ((ratio < t) & (ratio >= t - ulp)).any() and ((ratio >= t) & (ratio <= t + ulp)).any() and (ratio == t).any(), p


def test_kitti_sums_unchanged_by_the_metric_pixel_refactor():
    """``ge_depth_metrics`` on a case of test_eval_device_gpu.py: the sums equal ``sums_f64`` as before."""
    from gedepth_amd import kernels
    rng = np.random.default_rng(0)
    H, W, top, left, Hc, Wc = 40, 530, 2, 9, 37, 515
    raw = rng.integers(257, 20400, (H, W)).astype(np.uint16)
    raw[rng.random((H, W)) < 0.25] = 0
    g = R.window(raw, top, left, Hc, Wc)
    pred = np.where(g > 0, g * rng.uniform(0.5, 2.0, (Hc, Wc)), 5.0).astype(np.float32)
    rect = (int(0.40810811 * Hc), int(0.99189189 * Hc), int(0.03594771 * Wc), int(0.96405229 * Wc))
    out = torch.zeros(10, device='cuda', dtype=torch.float64)
    kernels.depth_metric_sums(torch.from_numpy(pred).cuda(), torch.from_numpy(raw).cuda(), top, left, rect, 256, 1e-3, 80, out)
    m = R.mask_of(g, rect, 1e-3, 80)
    _assert_sums(out.cpu().numpy(), R.sums_f64(g[m], pred[m]), 'kitti garg-rect')


def test_resized_wrapper_argument_errors():
    from gedepth_amd import kernels
    pred, gt = torch.ones(5, 7, device='cuda'), torch.ones(13, 18, device='cuda')
    out = torch.zeros(10, device='cuda', dtype=torch.float64)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums_resized(pred, gt.cpu(), *LIMITS, out)
    with pytest.raises(TypeError):
        kernels.depth_metric_sums_resized(pred.double(), gt, *LIMITS, out)
    with pytest.raises(ValueError, match='ten float64'):
        kernels.depth_metric_sums_resized(pred, gt, *LIMITS, torch.zeros(2, 10, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError, match='pred must be'):
        kernels.depth_metric_sums_resized(pred[None, None], gt, *LIMITS, out)
    kernels.depth_metric_sums_resized(pred[None], gt, *LIMITS, out)                   # (1, h, w) is taken
    assert out.cpu().numpy()[0] == 13 * 18


# ------------------------------------------------------------------------------------------------ the front end
def _frame_tree(root, H, W, seed):
    """One CAMERA_01 frame of (H, W) with a ground depth that holds negatives and values beyond 250."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    rgb_dir, d_dir, pe_dir = (os.path.join(root, *p) for p in (('000001', 'rgb', 'CAMERA_01'), ('000001', 'depth', 'CAMERA_01'), ('pe', 'CAMERA_01')))
    for d in (rgb_dir, d_dir, pe_dir):
        os.makedirs(d, exist_ok=True)
    pe = rng.uniform(-20, 320, (H, W)).astype(np.float32)
    pe[0, 0], pe[-1, -1], pe[1, 1] = 250.0, 250.5, 0.0
    np.savez(os.path.join(pe_dir, 'ddad_pe.npz'), pe=pe)
    Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(rgb_dir, '0.png'))
    np.savez(os.path.join(d_dir, '0.npz'), depth=np.zeros((H, W), np.float32))
    split = os.path.join(root, 'split.txt')
    with open(split, 'w') as fh:
        fh.write(f'{os.path.join(rgb_dir, "0.png")} {os.path.join(d_dir, "0.npz")}\n')
    return split, os.path.join(rgb_dir, '0.png'), pe


def _test_pipeline(pe_root, shape):
    from gedepth_amd.mmrt.config import Config
    out = []
    for t in Config.fromfile(os.path.join(CFG, 'depthformer_a_ddad.py')).data.test.pipeline:
        t = dict(t)
        if t['type'] == 'LoadDDADImageFromFile':
            t['pe_root'] = pe_root
        if t['type'] == 'DDADResize':
            t['shape'] = shape
        if t['type'] == 'MultiScaleFlipAug':
            t['img_scale'] = shape
        out.append(t)
    return out


def _composition(bgr, pe, Hd, Wd):
    """What the training pipeline runs (DDADGPUPipeline._front, then Normalize with the colour augmentation off), kernel by kernel."""
    from gedepth_amd import hip
    H, W = bgr.shape[:2]
    img = torch.empty(5, Hd, Wd, device='cuda')
    hip.call('ge_aug_area_u8', hip.ptr(bgr), hip.ptr(img), H, W, Hd, Wd, hip.stream())
    clamped = pe.clone()
    clamped[clamped > 250] = 0
    clamped[clamped < 0] = 0
    src = torch.stack((clamped, pe)).contiguous()
    hip.call('ge_aug_resize', hip.ptr(src), hip.ptr(img[3:5]), 2, H, W, Hd, Wd, 0, hip.stream())
    out = torch.empty(5, Hd, Wd, device='cuda')
    m, s = (ctypes.c_double * 3)(*[float(np.float32(v)) for v in MEAN]), (ctypes.c_double * 3)(*[float(np.float32(v)) for v in STD])
    hip.call('ge_aug_color_normalize', hip.ptr(img), hip.ptr(out), Hd, Wd, 0, 1.0, 1.0, None, ctypes.cast(m, ctypes.c_void_p),
             ctypes.cast(s, ctypes.c_void_p), 250.0, 1, hip.stream())
    return out


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('frame,shape', [((96, 160), (48, 80)), ((38, 61), (12, 20))], ids=['integer', 'fractional'])
def test_front_end_vs_training_kernels_and_host_pipeline(monkeypatch, tmp_path, frame, shape, poison):
    from gedepth_amd import eval_kernels, hip, kernels
    from gedepth_amd.depth.apis.inference import _decode
    from gedepth_amd.depth.datasets import build_dataset
    root = str(tmp_path)
    split, path, pe = _frame_tree(root, *frame, seed=sum(frame))
    assert (pe < 0).any() and (pe > 250).any()
    host = build_dataset(dict(type='DDADDataset', pipeline=_test_pipeline(os.path.join(root, 'pe'), shape), split=split, max_depth=200,
                              cameras=['CAMERA_01']), dict(test_mode=True))[0]
    ref = host['img'][0].float()
    assert tuple(ref.shape) == (5,) + shape
    mean, std = [float(np.float32(v)) for v in MEAN], [float(np.float32(v)) for v in STD]
    guard = memguard.Guard(poison)
    guard.install(monkeypatch, [eval_kernels], binding=hip)
    bgr, d_pe = guard.framed(torch.from_numpy(_decode(path)).cuda()), guard.framed(torch.from_numpy(pe).cuda())
    out = guard.proxy.empty(1, 5, *shape, device='cuda', dtype=torch.float32)
    kernels.infer_front_ddad(bgr, d_pe, out, mean, std, True, 250.0, 250.0)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_infer_front_ddad']
    want = _composition(bgr, d_pe, *shape)
    assert torch.equal(out[0], want), 'the front end must be bit-equal to ge_aug_area_u8 + nearest + Normalize'
    got = out[0].cpu()
    for c in (3, 4):                                                  # the bounds of test_ddad_device_pipeline_matches_host_pipeline
        err = (got[c] - ref[c]).abs()
        assert err.max().item() <= 1e-5 * max(1.0, ref[c].abs().max().item()), (c, err.max().item())
    err = (got[:3] - ref[:3]).abs()
    print(f'[front {frame} -> {shape}] colour: max {err.max().item():.2e}, {(err > 1e-5).float().mean().item():.2e} of the pixels differ')
    assert err.max().item() <= 0.0176 and (err > 1e-5).float().mean().item() <= 5e-3
    assert (got[3] == 0).any() and (got[3] > 0).any() and (got[4] < 0).any() and (got[4] > 250).any()


# ------------------------------------------------------------------------------------------------ engine and loop, on the toy tree
def _exact_variants(model):
    for m in model.modules():
        if hasattr(m, 'kernel_variant'):
            m.kernel_variant = 1
    return model


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """Random-init depthformer_a_ddad.py at Swin-T width (the scaling of depthformer_swint_a.py), the toy DDAD tree (96 x 160 frames),
    DDADResize to (48, 80); cameras as in the config, so CAMERA_01 and CAMERA_05 with two frames each."""
    from test_dataset_cpu import _make_toy_ddad
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    root = str(tmp_path_factory.mktemp('ddad_device_eval'))
    split = _make_toy_ddad(root, frames=2, seed=5)
    cfg = Config.fromfile(os.path.join(CFG, 'depthformer_a_ddad.py'))
    swin_t, rev = [64, 96, 192, 384, 768], [768, 384, 192, 96, 64]
    cfg.model.pretrained = None
    cfg.model.backbone.update(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24])
    cfg.model.neck.update(in_channels=swin_t, out_channels=swin_t)
    cfg.model.pe_mask_neck.in_channels = rev
    cfg.model.dynamic_pe_neck.in_channels = rev
    cfg.model.decode_head.update(in_channels=swin_t, up_sample_channels=swin_t)
    cfg.data.test.pipeline = _test_pipeline(os.path.join(root, 'pe'), (48, 80))
    cfg.data.test.split = split
    torch.manual_seed(0)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model.cfg = cfg
    model = _exact_variants(model.cuda().eval())
    ds = build_dataset(cfg.data.test, dict(test_mode=True))
    assert [i['ann']['depth_map'].split('/')[-2] for i in ds.img_infos] == ['CAMERA_01', 'CAMERA_01', 'CAMERA_05', 'CAMERA_05']
    return model, ds, (lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False))


@pytest.fixture(scope='module')
def host_maps(toy):
    """The maps of the host loop (host test pipeline -> ``simple_test``), computed once."""
    from gedepth_amd.depth.apis.test import single_gpu_test
    model, ds, loader = toy
    maps = single_gpu_test(model, loader())
    assert len(maps) == 4 and all(m.shape == (1, 48, 80) and m.dtype == np.float32 for m in maps)
    return maps


def _rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)).max())


def test_engine_eager_vs_simple_test(toy, host_maps):
    """The engine's eager map against ``model.simple_test`` through the host pipeline, per pixel and relative.  Measured on an MI355X:
    1.8e-6 .. 3.3e-6 on the four frames in two runs; the bound is ``ENGINE_EPS`` = 2e-4, the figure of the KITTI flip-TTA engine.  The
    front end's input must equal the host pipeline's tensor in every pixel (asserted below, on each frame), so what is measured is the
    forward's own run-to-run difference: two eager runs of one frame differ by 1.7e-6 .. 3.5e-6 relative per pixel, from the library's
    fp32 convolutions (test_graph_replay_follows_the_camera_height has the figures and the module where it starts)."""
    from gedepth_amd.depth.apis.inference import DepthInferencer
    model, ds, _ = toy
    eng = DepthInferencer(model)
    assert eng.static_in.shape == (1, 5, 48, 80) and eng.static_out.shape == (1, 48, 80) and eng.static_height.shape == (1,)
    worst = 0.0
    for i, info in enumerate(ds.img_infos):
        got = eng(info['filename'], graph=False)
        assert torch.equal(eng.static_in[0].cpu(), ds[i]['img'][0].float()), f'frame {i}: the front end must give the host pipeline\'s input'
        assert got.shape == (1, 48, 80) and got.dtype == np.float32 and np.isfinite(got).all()
        worst = max(worst, _rel(got, host_maps[i]))
        print(f'[engine frame {i}] eager vs simple_test: largest relative difference {_rel(got, host_maps[i]):.2e}')
    assert eng.captures == 0 and worst <= ENGINE_EPS
    with pytest.raises(ValueError, match='frames of'):
        eng(np.zeros((100, 160, 3), np.uint8), camera='CAMERA_01')                      # a new frame size
    with pytest.raises(ValueError, match='CAMERA_01, CAMERA_05'):
        eng(np.zeros((96, 160, 3), np.uint8))                                           # no path, no camera
    with pytest.raises(ValueError, match='CAMERA_07'):
        eng(np.zeros((96, 160, 3), np.uint8), camera='CAMERA_07')


@contextlib.contextmanager
def _reproducible_convolutions():
    """The fp32 convolutions of the eval forward go to the convolution library, whose default algorithm at these shapes is not
    bit-reproducible; asked for deterministic algorithms, the whole forward is.  The flag is read when a convolution is launched or
    captured, so an engine built and used inside this block runs and replays reproducible convolutions only."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def test_graph_replay_follows_the_camera_height(toy, monkeypatch):
    """One graph for every camera: a replayed CAMERA_05 frame equals its own eager result within the replay bound (1e-6 of the maximum)
    and differs from the replay computed with CAMERA_01's height, which a height baked into the graph could not.  The heights are set
    1.0 m apart for this test, so that the effect is large: the other height moves the map by 65 m (maximum 78 m).

    The forward's own noise, measured first: with the library's default convolution algorithms two EAGER runs of the same frame differ
    by 0.3e-6 .. 1.4e-6 of the map's maximum (2.7e-5 .. 1.1e-4 m of 78.5 m, seven pairs in three processes on an MI355X; 1.2e-6 ..
    2.6e-6 relative per pixel), and a replay differs from an eager run by as much (2.3e-5 .. 6.1e-5 m, four replays).  That is the size
    of the replay bound itself, so a comparison between two such runs says nothing about the graph.  Module by module, two runs on the
    same static input first differ in the output of the library's fp32 3 x 3 convolution of ``neck.trans_fusion[2]`` (2.4e-7 at a magnitude of 2.2)
    and grow through the decoder's convolutions (4.3e-6 at 7.0); every other module, the project's kernels among them, repeats its
    bits.  With deterministic convolution algorithms (_reproducible_convolutions) no module's output differs between two runs, four
    eager runs are bit-identical, and so are four replays and the eager run: measured difference 0.  The replay comparison therefore
    runs there, on the bound as it stands, with nothing of the noise in it; the noise of the default algorithms is printed and held
    below ``ENGINE_EPS`` of the maximum, which it would have to stay below for the loop comparisons anyway."""
    from gedepth_amd.depth.apis.inference import DepthInferencer, inference_depther
    from gedepth_amd.depth.datasets.pipelines import loading
    monkeypatch.setattr(loading, '_DDAD_CAMERA_HEIGHT', {'CAMERA_01': 1.2, 'CAMERA_05': 2.2, 'CAMERA_06': 1.53, 'CAMERA_09': 1.53})
    model, ds, _ = toy
    f01, f05 = ds.img_infos[0]['filename'], ds.img_infos[2]['filename']
    eng = DepthInferencer(model)
    a, b = eng(f05, graph=False), eng(f05, graph=False)
    noise = np.abs(a - b).max() / np.abs(a).max()
    print(f'[heights] default convolution algorithms: two eager runs differ by {noise:.2e} of the maximum {np.abs(a).max():.1f}')
    assert noise <= ENGINE_EPS
    with _reproducible_convolutions():
        eng = DepthInferencer(model)
        eager05 = eng(f05, graph=False)
        eager05_as01 = eng(f05, graph=False, camera='CAMERA_01')
        for _ in range(2):
            eng(f01)                                                                    # warm-up: CAMERA_01's height is in the buffer ...
        first = eng(f01)                                                                # ... when the graph is captured
        assert eng.captures == 1
        replay05 = eng(f05)
        replay05_as01 = eng(f05, camera='CAMERA_01')
        assert eng.captures == 1 and float(eng.static_height.cpu()) == np.float32(1.2)
    tol = 1e-6 * np.abs(eager05).max()
    print(f'[heights] reproducible convolutions: replay vs eager {np.abs(replay05 - eager05).max():.2e} and '
          f'{np.abs(replay05_as01 - eager05_as01).max():.2e} (tol {tol:.2e}), bit-identical {np.array_equal(replay05, eager05)}; '
          f'other height moves it by {np.abs(replay05 - replay05_as01).max():.2e}')
    assert np.abs(replay05 - eager05).max() <= tol and np.abs(replay05_as01 - eager05_as01).max() <= tol
    assert np.abs(replay05 - replay05_as01).max() > 100 * tol, 'the camera height must reach a replayed graph'
    assert np.abs(eager05 - a).max() <= ENGINE_EPS * np.abs(a).max()                    # the same map as with the default algorithms
    assert np.isfinite(first).all()
    monkeypatch.undo()
    model.__dict__.pop('_ge_inferencers', None)
    out = inference_depther(model, [f01, f05], graph=False)                             # cameras from the paths
    assert len(out) == 2 and all(o.shape == (1, 48, 80) and o.dtype == np.float32 for o in out)
    model.__dict__.pop('_ge_inferencers', None)


def test_back_to_back_frames_each_get_their_own_camera_height(toy, monkeypatch):
    """The camera height travels through one reused pinned buffer and a non-blocking copy: six replayed frames, alternating two cameras,
    queued without any host synchronisation between them.  Each call's map (and height) is cloned on the caller's stream right behind
    it and must equal, bit for bit, the map the same engine gives that frame with ``to_host=True``.  A pinned buffer overwritten before
    its copy has run would give a frame the other camera's height, which moves the map by more than 100 times the replay bound
    (test_graph_replay_follows_the_camera_height); bit equality needs the reproducible convolutions, as there."""
    from gedepth_amd.depth.apis.inference import DepthInferencer
    from gedepth_amd.depth.datasets.pipelines import loading
    heights = {'CAMERA_01': 1.2, 'CAMERA_05': 2.2, 'CAMERA_06': 1.53, 'CAMERA_09': 1.53}
    monkeypatch.setattr(loading, '_DDAD_CAMERA_HEIGHT', heights)
    model, ds, _ = toy
    frames = [(ds.img_infos[0]['filename'], 'CAMERA_01'), (ds.img_infos[2]['filename'], 'CAMERA_05')]
    order = [0, 1, 0, 1, 0, 1]
    with _reproducible_convolutions():
        eng = DepthInferencer(model)
        for _ in range(eng.WARMUP + 1):
            eng(frames[0][0])
        assert eng.captures == 1
        want = [eng(f) for f, _ in frames]                                              # replays; to_host=True synchronises
        maps, seen = [], []
        for k in order:
            out = eng(frames[k][0], to_host=False)
            assert out is eng.static_out
            maps.append(out.clone())
            seen.append(eng.static_height.clone())
        torch.cuda.synchronize()
        assert eng.captures == 1 and eng.replays == 1 + len(want) + len(order)
    assert not np.array_equal(want[0], want[1])
    for call, (k, m, h) in enumerate(zip(order, maps, seen)):
        assert h.cpu().numpy().tolist() == [np.float32(heights[frames[k][1]])], f'call {call}: the height of {frames[k][1]}'
        assert np.array_equal(m.cpu().numpy(), want[k]), f'call {call}: not the map of its own frame and camera'


def _host_counted(ds, i):
    gt = np.load(ds.img_infos[i]['ann']['depth_map'])['depth'].astype(np.float32)
    return gt, D.mask_of(gt, *LIMITS)


def test_pre_eval_device_on_the_maps_of_the_host_loop(toy, host_maps):
    """``pre_eval_device`` fed the maps the host loop returned: the engine is out of this comparison.  Counts equal the restatement; the
    host path gets the near-threshold allowance of ``HOST_BAND``."""
    from gedepth_amd.depth.core import metrics_from_sums
    model, ds, _ = toy
    sums = torch.full((len(host_maps) + 1, 10), -7.0, device='cuda', dtype=torch.float64)
    for i, m in enumerate(host_maps):
        ds.pre_eval_device(torch.from_numpy(m).cuda(), i, sums[i])
    rows = sums.cpu().numpy()
    assert (rows[-1] == -7.0).all()
    for i, m in enumerate(host_maps):
        gt, mask = _host_counted(ds, i)
        assert rows[i][0] == mask.sum() > 1000
        _assert_sums(rows[i], R.sums_f64(gt[mask], D.resize_f32(m[0], *gt.shape)[mask]), f'frame {i}')
        host_pred = ds.pre_eval([m], [i])[1][0]                                        # the (1, H, W) map F.interpolate made
        _assert_vs_host(metrics_from_sums(rows[i]), gt[mask], host_pred[0][mask], f'frame {i}', D.HOST_BAND)
    with pytest.raises(TypeError):
        ds.pre_eval_device(torch.from_numpy(host_maps[0]), 0, sums[0])                  # a host map
    with pytest.raises(TypeError):
        ds.pre_eval_device(torch.from_numpy(host_maps[0]).cuda().double(), 0, sums[0])


def test_device_eval_loop_vs_host_loop(toy, host_maps):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    model, ds, loader = toy
    host = single_gpu_test(model, loader(), pre_eval=True)
    model.__dict__.pop('_ge_inferencers', None)
    dev = single_gpu_test(model, loader(), pre_eval=True, device_eval=True)
    eng = model._ge_inferencers[False]
    assert eng.captures == 1 and len(dev) == len(host) == 4                              # two eager frames, the capture, a replay
    assert all(isinstance(t, tuple) and len(t) == 9 for t in dev)
    for i, (d, h) in enumerate(zip(dev, host)):
        gt, mask = _host_counted(ds, i)
        host_pred = ds.pre_eval([host_maps[i]], [i])[1][0][0]
        # a prediction that moves by eps relative moves its ratio by eps / (1 - eps): twice eps covers it, as in test_eval_device_gpu.py
        eps = ENGINE_EPS + D.HOST_BAND
        _assert_vs_host(d, gt[mask], host_pred[mask], f'loop frame {i}', eps, band=2 * eps)
    summary = ds.evaluate(dev)                                                           # the list works where pre_eval's does
    assert set(summary) == set(METRIC_NAMES) and all(np.isfinite(v) for v in summary.values())
    model.__dict__.pop('_ge_inferencers', None)


def test_device_eval_refuses_a_dataset_of_the_other_protocol(toy):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    from gedepth_amd.mmrt.config import Config
    model, ds, loader = toy

    class KITTILoader:
        dataset = KITTIDataset.__new__(KITTIDataset)                                     # bare: no attribute may be touched
        batch_sampler = [[0]]
    with pytest.raises(NotImplementedError, match=r'KITTIDataset.*kitti.*ddad'):
        single_gpu_test(model, KITTILoader(), pre_eval=True, device_eval=True)
    kitti_model = types.SimpleNamespace(cfg=Config.fromfile(os.path.join(CFG, 'depthformer_swint_v.py')), eval=lambda: None)
    with pytest.raises(NotImplementedError, match=r'DDADDataset.*ddad.*kitti'):
        single_gpu_test(kitti_model, loader(), pre_eval=True, device_eval=True)
