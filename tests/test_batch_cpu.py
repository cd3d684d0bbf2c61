"""The batched KITTI entry points, the parts that need no GPU: the second table of headers and its binding, the ``GeBatchFrame`` mirror,
argument validation of the three entry points (every check comes before a launch), and the argument errors of ``inference_depther(batch=)``
and ``tools/test.py --eval-batch``."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from gedepth_amd import batch_kernels as B
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
BAD_ARG, UNSUPPORTED = 10001, 10002
P = 4096                                                             # a fake non-null, 16-byte aligned pointer that is never followed


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


def test_extra_header_is_parsed_and_bound():
    assert hip.EXTRA_HEADERS == {'BATCH_SIGNATURES': 'gedepth_batch.h'}
    assert len(hip.HEADERS) == 5 and list(hip.HEADERS)[-1] == 'GROUND_SIGNATURES' and not set(hip.HEADERS) & set(hip.EXTRA_HEADERS)
    header = open(os.path.join(ROOT, 'include', 'gedepth_batch.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.BATCH_SIGNATURES) == {'ge_batch_frame_size', 'ge_infer_front_batch', 'ge_tta_merge_batch',
                                                     'ge_depth_metrics_batch', 'ge_depth_metrics_batch_workspace'}
    for table in hip.HEADERS:
        assert not set(hip.BATCH_SIGNATURES) & set(getattr(hip, table)), table
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.BATCH_SIGNATURES['ge_infer_front_batch'] == (i, [vp, i, vp, i, i, i, f, vp, vp, f, i, vp])
    assert hip.BATCH_SIGNATURES['ge_tta_merge_batch'] == (i, [vp, vp, i, i, i, vp])
    assert hip.BATCH_SIGNATURES['ge_depth_metrics_batch'] == (i, [vp, vp, i, i, i, i, i, i, i, f, f, f, vp, vp, vp])
    assert hip.BATCH_SIGNATURES['ge_depth_metrics_batch_workspace'] == (c.c_size_t, [i, i, i])
    assert hip.BATCH_SIGNATURES['ge_batch_frame_size'] == (c.c_size_t, [])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    for name, (res, args) in hip.BATCH_SIGNATURES.items():
        fn = getattr(hip.lib(), name)                                  # lib() has bound the second table too
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert hip.lib().ge_abi_version() == 7 and len(hip.SIGNATURES) == 102


def test_frame_struct_mirror_and_kernels_reexport():
    from gedepth_amd import kernels
    lib = hip.lib()
    assert ctypes.sizeof(B.GeBatchFrame) == lib.ge_batch_frame_size() == 32           # 8 of them: the 256-byte by-value table
    assert [n for n, _ in B.GeBatchFrame._fields_] == ['image', 'aux', 'H', 'W', 'top', 'left']
    t = B._table([(P, P + 16, 375, 1242, 23, 13), (P, None, 370, 1224, 18, 4)])
    assert (t[1].image, t[1].aux, t[1].H, t[1].W, t[1].top, t[1].left) == (P, None, 370, 1224, 18, 4) and t[0].aux == P + 16
    for name in ('infer_front_batch', 'tta_merge_batch', 'depth_metric_sums_batch'):
        assert getattr(kernels, name) is getattr(B, name)
    assert B.BATCH_MAX == 8
    # the workspace: n times the single-image one; 0 outside 1 .. 8
    one = lib.ge_depth_metrics_workspace(352, 1216)
    assert [lib.ge_depth_metrics_batch_workspace(n, 352, 1216) for n in (0, 1, 3, 8, 9)] == [0, one, 3 * one, 8 * one, 0]
    assert lib.ge_depth_metrics_batch_workspace(2, 0, 16) == 0


def _frames(n=2, image=P, aux=P, H=11, W=30, top=3, left=3):
    return B._table([(image, aux, H, W, top, left)] * n)


def test_front_batch_argument_validation_without_a_gpu():
    lib = hip.lib()
    m = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def run(frames='default', n=2, dst=P, Hc=8, Wc=24, views=2, mean=m, std=m):
        frames = _vp(_frames(max(n, 1) if 1 <= n <= 8 else 8)) if frames == 'default' else frames
        return lib.ge_infer_front_batch(frames, n, dst, Hc, Wc, views, 200.0, _vp(mean) if mean else None, _vp(std) if std else None, 200.0, 1,
                                        None)
    assert run(frames=None) == BAD_ARG and run(dst=None) == BAD_ARG and run(mean=None) == BAD_ARG and run(std=None) == BAD_ARG
    assert run(frames=_vp(_frames(image=None))) == BAD_ARG and run(frames=_vp(_frames(aux=None))) == BAD_ARG
    for n in (0, -1, 9):
        assert run(n=n) == BAD_ARG, n
    for views in (0, 3):
        assert run(views=views) == BAD_ARG
    assert run(Hc=0) == BAD_ARG and run(Wc=-4) == BAD_ARG
    assert run(frames=_vp(_frames(top=4))) == BAD_ARG                  # 4 + 8 > 11: the window leaves its frame
    assert run(frames=_vp(_frames(left=7))) == BAD_ARG                 # 7 + 24 > 30
    assert run(frames=_vp(_frames(top=-1))) == BAD_ARG
    # the second frame alone is wrong
    two = B._table([(P, P, 11, 30, 3, 3), (P, P, 9, 27, 2, 3)])
    assert run(frames=_vp(two)) == BAD_ARG
    assert run(Wc=22) == UNSUPPORTED and run(dst=P + 4) == UNSUPPORTED
    assert run(frames=_vp(_frames(aux=P + 2))) == UNSUPPORTED


def test_merge_batch_argument_validation_without_a_gpu():
    lib = hip.lib()

    def run(src=P, dst=P, n=2, H=5, W=8):
        return lib.ge_tta_merge_batch(src, dst, n, H, W, None)
    assert run(src=None) == BAD_ARG and run(dst=None) == BAD_ARG
    for n in (0, -3, 9):
        assert run(n=n) == BAD_ARG, n
    assert run(H=0) == BAD_ARG and run(W=0) == BAD_ARG
    assert run(W=6) == UNSUPPORTED and run(src=P + 4) == UNSUPPORTED and run(dst=P + 8) == UNSUPPORTED


def test_metrics_batch_argument_validation_without_a_gpu():
    lib = hip.lib()

    def run(pred=P, frames='default', n=2, Hc=8, Wc=24, rect=(0, 8, 0, 24), partials=P, sums=P):
        frames = _vp(_frames(max(n, 1) if 1 <= n <= 8 else 8, aux=None)) if frames == 'default' else frames
        return lib.ge_depth_metrics_batch(pred, frames, n, Hc, Wc, *rect, 256.0, 1e-3, 80.0, partials, sums, None)
    assert run(pred=None) == BAD_ARG and run(frames=None) == BAD_ARG and run(partials=None) == BAD_ARG and run(sums=None) == BAD_ARG
    assert run(frames=_vp(_frames(image=None, aux=None))) == BAD_ARG
    for n in (0, 9):
        assert run(n=n) == BAD_ARG, n
    assert run(frames=_vp(_frames(top=4, aux=None))) == BAD_ARG and run(frames=_vp(_frames(left=7, aux=None))) == BAD_ARG
    assert run(rect=(0, 9, 0, 24)) == BAD_ARG and run(rect=(0, 8, -1, 24)) == BAD_ARG      # the rectangle leaves the crop
    assert run(Wc=22, rect=(0, 8, 0, 22)) == UNSUPPORTED
    assert run(pred=P + 4) == UNSUPPORTED and run(sums=P + 4) == UNSUPPORTED and run(frames=_vp(_frames(image=P + 1, aux=None))) == UNSUPPORTED


def test_wrappers_refuse_a_wrong_frame_count_before_the_library():
    with pytest.raises(ValueError, match='1 .. 8'):
        B.infer_front_batch([], [], torch.zeros(2, 5, 8, 24), [], [], (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='1 .. 8'):
        B.tta_merge_batch(torch.zeros(18, 1, 5, 8), torch.zeros(9, 1, 5, 8))
    with pytest.raises(ValueError, match='1 .. 8'):
        B.depth_metric_sums_batch(torch.zeros(9, 8, 24), [torch.zeros(1)] * 9, [0] * 9, [0] * 9, (0, 8, 0, 24), 256, 1e-3, 80,
                                  torch.zeros(9, 10, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='MI355X only'):             # CPU tensors are not run
        B.tta_merge_batch(torch.zeros(4, 1, 5, 8), torch.zeros(2, 1, 5, 8))


def _cpu_model(cfg_name):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, cfg_name))
    cfg.model.pretrained = None
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.cfg = cfg
    return model.eval()


def test_inference_depther_batch_argument_errors_before_device_work():
    """A CPU model: any device work would raise something else (``torch.cuda.Stream``), so each error below comes before it."""
    from gedepth_amd.depth.apis import inference_depther
    from gedepth_amd.depth.apis.batch_inference import DECODE_WORKERS
    assert DECODE_WORKERS <= 4
    model = _cpu_model('depthformer_swint_v.py')
    frame = np.zeros((375, 1242, 3), np.uint8)
    pe = np.zeros((375, 1242), np.float32)
    with pytest.raises(ValueError, match=r'1 \.\. 8.*got 0'):
        inference_depther(model, [frame, frame], pe=pe, batch=0)
    with pytest.raises(ValueError, match=r'1 \.\. 8.*got 9'):
        inference_depther(model, [frame, frame], pe=pe, batch=9)
    with pytest.raises(ValueError, match='1 ground-depth maps for 2 frames'):
        inference_depther(model, [frame, frame], pe=[pe], batch=2)
    with pytest.raises(ValueError, match='no ground depth'):
        inference_depther(model, [frame, frame], batch=2)
    small = np.zeros((300, 1242, 3), np.uint8)
    with pytest.raises(ValueError, match='smaller than the KB crop'):
        inference_depther(model, [frame, small], pe=[pe, np.zeros((300, 1242), np.float32)], batch=2)
    ddad = _cpu_model('depthformer_v_ddad.py')
    with pytest.raises(NotImplementedError, match='DDAD'):
        inference_depther(ddad, [frame, frame], camera='CAMERA_01', batch=2)


def test_decode_ahead_keeps_order_and_runs_the_next_list_early():
    from gedepth_amd.depth.apis.batch_inference import decode_ahead
    started = []

    def job(k):
        def run():
            started.append(k)
            return k * k
        return run
    seen = []
    for part in decode_ahead([job(k) for k in range(5)], 2):
        seen.append((part, sorted(started)))
    assert [p for p, _ in seen] == [[0, 1], [4, 9], [16]]
    assert all(set(range(min(5, 2 * (k + 1)))) <= set(s) for k, (_, s) in enumerate(seen))     # the current list is done when it is handed out
    assert list(decode_ahead([], 3)) == []

    def boom():
        raise KeyError('frame 1')
    with pytest.raises(KeyError, match='frame 1'):
        list(decode_ahead([job(0), boom, job(2)], 2))


def _cli(name):
    spec = importlib.util.spec_from_file_location(f'tools_{name}_cli_batch', os.path.join(ROOT, 'tools', f'{name}.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_eval_batch_needs_device_eval():
    cli = _cli('test')
    cfg = os.path.join(CFG, 'depthformer_swint_v.py')
    with pytest.raises(ValueError, match='--eval-batch needs --device-eval'):
        cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--eval-batch', '2'])
    with pytest.raises(ValueError, match='1 .. 8'):
        cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--device-eval', '--eval-batch', '9'])
    with pytest.raises(ValueError, match='--ground-dir'):
        cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--device-eval', '--eval-batch', '2', '--ground-dir', 'd'])
    args = cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--device-eval', '--eval-batch', '4'])
    assert args.eval_batch == 4 and cli.parse_args([cfg]).eval_batch == 1


def test_eval_batch_without_device_eval_raises_in_the_loop():
    from gedepth_amd.depth.apis.test import single_gpu_test
    with pytest.raises(NotImplementedError, match='device_eval=True'):
        single_gpu_test(torch.nn.Identity(), None, pre_eval=True, eval_batch=2)
