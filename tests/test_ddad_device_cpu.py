"""The DDAD device protocol, the parts that need no GPU: the third header and its binding, ``ddad_front_spec`` / ``front_spec``, the
camera rule of ``inference_depther``, argument validation of the two entry points, and the gap between the float32 restatement of the
kernel's resampling (tests/ddad_ref.py) and ATen's CPU ``F.interpolate``.

Measured gap (torch 2.x CPU, values 1 .. 150): the largest relative difference over tests/ddad_ref.py's geometries is 2.7e-7, and
3.4e-7 on 384 x 640 -> 1216 x 1936; the tests that compare the kernel with the host path allow 1e-6 (``ddad_ref.HOST_BAND``)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ddad_ref as D
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
BAD_ARG, UNSUPPORTED = 10001, 10002


def _cfg(name):
    from gedepth_amd.mmrt.config import Config
    return Config.fromfile(os.path.join(CFG, name))


def test_ddad_header_parses_and_library_exports_it():
    header = open(os.path.join(ROOT, 'include', 'gedepth_ddad.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.DDAD_SIGNATURES) == {'ge_infer_front_ddad', 'ge_depth_metrics_resized', 'ge_depth_metrics_resized_workspace'}
    assert not set(hip.DDAD_SIGNATURES) & (set(hip.SIGNATURES) | set(hip.EVAL_SIGNATURES))
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.DDAD_SIGNATURES['ge_depth_metrics_resized'] == (i, [vp, i, i, vp, i, i, f, f, vp, vp, vp])
    assert hip.DDAD_SIGNATURES['ge_depth_metrics_resized_workspace'] == (c.c_size_t, [i, i])
    assert hip.DDAD_SIGNATURES['ge_infer_front_ddad'] == (i, [vp, vp, vp, i, i, i, i, f, vp, vp, f, i, vp])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    for name, (res, args) in hip.DDAD_SIGNATURES.items():
        fn = getattr(hip.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_argument_validation_without_a_gpu():
    """Every check comes before a launch, so fake non-null pointers are never followed."""
    lib = hip.lib()
    p = 4096

    def run(pred=p, gt=p, h=4, w=4, H=9, W=11, partials=p, sums=p):
        return lib.ge_depth_metrics_resized(pred, h, w, gt, H, W, 1e-3, 200.0, partials, sums, None)
    for null in ('pred', 'gt', 'partials', 'sums'):
        assert run(**{null: None}) == BAD_ARG, null
    for size in ('h', 'w', 'H', 'W'):
        assert run(**{size: 0}) == BAD_ARG and run(**{size: -3}) == BAD_ARG, size
    assert run(pred=p + 2) == UNSUPPORTED and run(gt=p + 1) == UNSUPPORTED and run(partials=p + 4) == UNSUPPORTED and run(sums=p + 4) == UNSUPPORTED
    assert lib.ge_depth_metrics_resized_workspace(0, 5) == 0 and lib.ge_depth_metrics_resized_workspace(5, -1) == 0
    assert lib.ge_depth_metrics_resized_workspace(1, 1) == 80
    assert lib.ge_depth_metrics_resized_workspace(1216, 1936) % 80 == 0

    def front(bgr=p, pe=p, dst=p, H=38, W=61, Hd=12, Wd=20, mean=p, std=p):
        return lib.ge_infer_front_ddad(bgr, pe, dst, H, W, Hd, Wd, 250.0, mean, std, 250.0, 1, None)
    for null in ('bgr', 'pe', 'dst', 'mean', 'std'):
        assert front(**{null: None}) == BAD_ARG, null
    for size in ('H', 'W', 'Hd', 'Wd'):
        assert front(**{size: 0}) == BAD_ARG, size
    assert front(Wd=18) == UNSUPPORTED and front(dst=p + 8) == UNSUPPORTED          # Wd % 4, 16-byte dst
    assert front(Hd=39) == UNSUPPORTED and front(Wd=64) == UNSUPPORTED              # the area filter only shrinks


def test_wrappers_refuse_cpu_tensors():
    import torch
    from gedepth_amd import kernels
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums_resized(torch.zeros(4, 4), torch.zeros(9, 11), 1e-3, 200, torch.zeros(10, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.infer_front_ddad(torch.zeros(38, 61, 3, dtype=torch.uint8), torch.zeros(38, 61), torch.zeros(1, 5, 12, 20), (0, 0, 0), (1, 1, 1))


@pytest.mark.parametrize('name', ['depthformer_v_ddad.py', 'depthformer_a_ddad.py'])
def test_ddad_front_spec_reads_the_config(name):
    from gedepth_amd.depth.apis.inference import ddad_front_spec, front_spec
    s = ddad_front_spec(_cfg(name))
    assert (s['protocol'], s['height'], s['width'], s['views']) == ('ddad', 384, 640, 1)
    assert s['pe_max'] == 250.0 and s['depth_scale'] == 250.0 and s['to_rgb']
    assert s['mean'] == [float(np.float32(v)) for v in (123.675, 116.28, 103.53)]
    assert s['std'] == [float(np.float32(v)) for v in (58.395, 57.12, 57.375)]
    assert s['pe_root'] == os.path.join('data', 'DDAD', 'pe_public_debug')
    assert front_spec(_cfg(name)) == s
    cfg = _cfg(name)
    cfg.data.test.pipeline[0]['pe_root'] = '/somewhere/pe'
    cfg.data.test.pipeline[1]['shape'] = (48, 80)
    s = ddad_front_spec(cfg)
    assert (s['height'], s['width'], s['pe_root']) == (48, 80, '/somewhere/pe')


def test_ddad_front_spec_refuses_other_pipelines():
    from gedepth_amd.depth.apis.inference import ddad_front_spec
    with pytest.raises(NotImplementedError, match='KBCrop'):
        ddad_front_spec(_cfg('depthformer_swint_v.py'))
    cfg = _cfg('depthformer_a_ddad.py')
    aug = next(t for t in cfg.data.test.pipeline if t['type'] == 'MultiScaleFlipAug')
    aug['flip'] = True
    with pytest.raises(NotImplementedError, match='flip=True'):
        ddad_front_spec(cfg)
    aug['flip'] = False
    aug['transforms'].insert(0, dict(type='Resize', keep_ratio=True))
    with pytest.raises(NotImplementedError, match='Resize'):
        ddad_front_spec(cfg)
    del aug['transforms'][0]
    ddad_front_spec(cfg)
    cfg.data.test.pipeline.insert(1, dict(type='LoadDDADCamIntrinsic'))
    with pytest.raises(NotImplementedError, match='LoadDDADCamIntrinsic'):
        ddad_front_spec(cfg)
    del cfg.data.test.pipeline[1]
    cfg.data.test.pipeline[1]['depth'] = True
    with pytest.raises(NotImplementedError, match='DDADResize'):
        ddad_front_spec(cfg)
    cfg.data.test.pipeline[1]['depth'] = False
    cfg.data.test.pipeline[0]['USE_DYNAMIC_PE'] = False
    with pytest.raises(NotImplementedError, match='LoadDDADImageFromFile'):
        ddad_front_spec(cfg)


def test_front_spec_dispatches_on_the_pipeline():
    from gedepth_amd.depth.apis.inference import front_spec, kitti_front_spec
    for name in ('depthformer_swint_v.py', 'depthformer_a.py'):
        s = front_spec(_cfg(name))
        assert s['protocol'] == 'kitti' and (s['height'], s['width'], s['views']) == (352, 1216, 2)
        assert {k: v for k, v in s.items() if k != 'protocol'} == kitti_front_spec(_cfg(name))
    assert front_spec(_cfg('depthformer_v_ddad.py'))['protocol'] == 'ddad'
    with pytest.raises(NotImplementedError, match='DDADResize'):                    # unchanged: the KITTI spec names the DDAD steps
        kitti_front_spec(_cfg('depthformer_v_ddad.py'))


def test_inference_depther_needs_a_camera_before_any_device_work():
    """A CPU model: any device work would fail differently."""
    from gedepth_amd.depth.apis import inference_depther, init_depther
    model = init_depther(os.path.join(CFG, 'depthformer_v_ddad.py'), device='cpu')
    frame, pe = np.zeros((1216, 1936, 3), np.uint8), np.zeros((1216, 1936), np.float32)
    with pytest.raises(NotImplementedError, match=r'DDADResize.*pass camera='):
        inference_depther(model, frame, pe=pe)
    with pytest.raises(NotImplementedError, match=r'DDADResize.*pass camera='):
        inference_depther(model, '/data/000001/rgb/CAMERA_07/0.png', pe=pe)          # a camera without a known height
    with pytest.raises(ValueError, match=r'CAMERA_07.*CAMERA_01, CAMERA_05, CAMERA_06, CAMERA_09'):
        inference_depther(model, frame, pe=pe, camera='CAMERA_07')
    with pytest.raises(ValueError, match='2 cameras for 1 frames'):
        inference_depther(model, frame, pe=pe, camera=['CAMERA_01', 'CAMERA_05'])


def test_restatement_identity_and_degenerate_axes():
    rng = np.random.default_rng(0)
    pred = rng.uniform(1, 150, (8, 12)).astype(np.float32)
    assert np.array_equal(D.resize_f32(pred, 8, 12), pred)                          # every w1 == 0
    assert np.array_equal(D.resize_f32(pred, 1, 1), pred[:1, :1])                   # scale == 0
    assert np.array_equal(D.resize_f32(pred, 1, 12), pred[:1]) and np.array_equal(D.resize_f32(pred, 8, 1), pred[:, :1])


@pytest.mark.parametrize('geom', D.GEOMETRIES, ids=lambda g: f'{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}')
def test_restatement_vs_aten_gap(geom):
    """Keeps ``HOST_BAND`` honest if torch changes: the largest relative difference between the restatement and ``F.interpolate``."""
    (h, w), (H, W) = geom
    worst = 0.0
    for seed in range(4):
        pred = np.random.default_rng(seed).uniform(1, 150, (h, w)).astype(np.float32)
        a, b = D.resize_f32(pred, H, W), D.resize_host(pred, H, W)
        worst = max(worst, float((np.abs(a.astype(np.float64) - b) / np.abs(b)).max()))
    print(f'[{h}x{w} -> {H}x{W}] restatement vs F.interpolate: largest relative difference {worst:.2e}')
    assert worst <= D.HOST_BAND
