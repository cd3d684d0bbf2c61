"""The batched DDAD entry points, the parts that need no GPU: the eighth table of headers and its binding, argument validation of the two
entry points (every check comes before a launch, every bad argument before anything unsupported), the workspace sizes, the argument errors
of ``BatchDDADInferencer`` and of ``eval_batch`` with a DDAD split (before any device work: the models are CPU models), and
``tools/test.py --eval-batch`` with a DDAD config and the DDAD tree of ``tools/benchmark_eval.py``."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from gedepth_amd import batch_kernels as B
from gedepth_amd import ddad_batch_kernels as DB
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
BAD_ARG, UNSUPPORTED = 10001, 10002
P = 4096                                                             # a fake non-null, 16-byte aligned pointer that is never followed
OTHER_TABLES = ('HEADERS', 'EXTRA_HEADERS', 'SCENE_HEADERS', 'STRATA_HEADERS', 'NECK_HEADERS', 'ERROR_HEADERS', 'ACCUM_HEADERS')


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


def _lib():
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    return hip.lib()


# ------------------------------------------------------------------------------------------------ header table, binding
def test_ddad_batch_header_is_parsed_into_its_own_table():
    assert hip.DDAD_BATCH_HEADERS == {'DDAD_BATCH_SIGNATURES': 'gedepth_ddad_batch.h'}
    header = open(os.path.join(ROOT, 'include', 'gedepth_ddad_batch.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.DDAD_BATCH_SIGNATURES) == {'ge_infer_front_ddad_batch', 'ge_depth_metrics_resized_batch',
                                                          'ge_depth_metrics_resized_batch_workspace'}
    for group in OTHER_TABLES:
        for table in getattr(hip, group):
            assert table != 'DDAD_BATCH_SIGNATURES' and not declared & set(getattr(hip, table)), table
    # the headers whose symbol sets earlier tests pin keep them
    assert set(hip.DDAD_SIGNATURES) == {'ge_infer_front_ddad', 'ge_depth_metrics_resized', 'ge_depth_metrics_resized_workspace'}
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.DDAD_BATCH_SIGNATURES['ge_infer_front_ddad_batch'] == (i, [vp, i, vp, i, i, f, vp, vp, f, i, vp])
    assert hip.DDAD_BATCH_SIGNATURES['ge_depth_metrics_resized_batch'] == (i, [vp, i, i, vp, i, f, f, vp, vp, vp])
    assert hip.DDAD_BATCH_SIGNATURES['ge_depth_metrics_resized_batch_workspace'] == (c.c_size_t, [i, i, i])
    lib = _lib()
    for name, (res, args) in hip.DDAD_BATCH_SIGNATURES.items():
        fn = getattr(lib, name)                                        # lib() has bound the eighth table too
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.ge_abi_version() == 7                                   # the versioned ABI does not move


def test_kernels_reexport_and_workspace_sizes():
    from gedepth_amd import kernels
    for name in ('infer_front_ddad_batch', 'depth_metric_sums_resized_batch'):
        assert getattr(kernels, name) is getattr(DB, name)
    assert DB.BATCH_MAX == 8
    lib = _lib()
    one = lib.ge_depth_metrics_resized_workspace(1216, 1936)
    assert one > 0 and one % 80 == 0
    # n times the single-image one (the same block partition per image); 0 outside 1 .. 8 and for non-positive sizes
    assert [lib.ge_depth_metrics_resized_batch_workspace(n, 1216, 1936) for n in (-1, 0, 1, 3, 8, 9)] == [0, 0, one, 3 * one, 8 * one, 0]
    assert lib.ge_depth_metrics_resized_batch_workspace(2, 0, 16) == 0 and lib.ge_depth_metrics_resized_batch_workspace(2, 16, -1) == 0
    assert lib.ge_depth_metrics_resized_workspace(0, 16) == 0 and lib.ge_depth_metrics_resized_workspace(16, 0) == 0
    assert lib.ge_depth_metrics_batch_workspace(9, 16, 16) == 0 and lib.ge_depth_metrics_batch_workspace(0, 16, 16) == 0
    assert lib.ge_depth_metrics_resized_batch_workspace(1, 37, 61) == lib.ge_depth_metrics_resized_workspace(37, 61)


def _frames(n=2, image=P, aux=P, H=38, W=61, top=0, left=0):
    return B._table([(image, aux, H, W, top, left)] * n)


# ------------------------------------------------------------------------------------------------ argument validation
def test_front_ddad_batch_argument_validation_without_a_gpu():
    lib = _lib()
    m = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def run(frames='default', n=2, dst=P, Hd=12, Wd=20, mean=m, std=m):
        frames = _vp(_frames(max(n, 1) if 1 <= n <= 8 else 8)) if frames == 'default' else frames
        return lib.ge_infer_front_ddad_batch(frames, n, dst, Hd, Wd, 250.0, _vp(mean) if mean else None, _vp(std) if std else None, 250.0, 1,
                                             None)
    assert run(frames=None) == BAD_ARG and run(dst=None) == BAD_ARG and run(mean=None) == BAD_ARG and run(std=None) == BAD_ARG
    assert run(frames=_vp(_frames(image=None))) == BAD_ARG and run(frames=_vp(_frames(aux=None))) == BAD_ARG
    for n in (0, -1, 9):
        assert run(n=n) == BAD_ARG, n
    assert run(Hd=0) == BAD_ARG and run(Wd=-4) == BAD_ARG
    assert run(frames=_vp(_frames(H=0))) == BAD_ARG and run(frames=_vp(_frames(W=-3))) == BAD_ARG
    assert run(frames=_vp(_frames(top=1))) == BAD_ARG and run(frames=_vp(_frames(left=4))) == BAD_ARG and run(frames=_vp(_frames(top=-1))) == BAD_ARG
    two = B._table([(P, P, 38, 61, 0, 0), (P, None, 38, 61, 0, 0)])    # the second frame alone is wrong
    assert run(frames=_vp(two)) == BAD_ARG
    assert run(Hd=39) == UNSUPPORTED and run(Wd=64) == UNSUPPORTED     # the area filter only shrinks
    assert run(frames=_vp(B._table([(P, P, 38, 61, 0, 0), (P, P, 11, 61, 0, 0)]))) == UNSUPPORTED       # ... in every frame
    assert run(Wd=18) == UNSUPPORTED and run(dst=P + 4) == UNSUPPORTED and run(frames=_vp(_frames(aux=P + 2))) == UNSUPPORTED
    # a bad argument is reported before anything unsupported
    assert run(Wd=18, frames=_vp(_frames(top=1))) == BAD_ARG and run(dst=P + 4, n=9) == BAD_ARG and run(Hd=39, mean=None) == BAD_ARG


def test_resized_batch_argument_validation_without_a_gpu():
    lib = _lib()

    def run(pred=P, h=12, w=20, frames='default', n=2, partials=P, sums=P):
        frames = _vp(_frames(max(n, 1) if 1 <= n <= 8 else 8, aux=None)) if frames == 'default' else frames
        return lib.ge_depth_metrics_resized_batch(pred, h, w, frames, n, 1e-3, 200.0, partials, sums, None)
    assert run(pred=None) == BAD_ARG and run(frames=None) == BAD_ARG and run(partials=None) == BAD_ARG and run(sums=None) == BAD_ARG
    assert run(frames=_vp(_frames(image=None, aux=None))) == BAD_ARG
    for n in (0, -2, 9):
        assert run(n=n) == BAD_ARG, n
    assert run(h=0) == BAD_ARG and run(w=-1) == BAD_ARG and run(frames=_vp(_frames(H=0))) == BAD_ARG
    assert run(frames=_vp(_frames(top=2))) == BAD_ARG and run(frames=_vp(_frames(left=1))) == BAD_ARG
    mixed = B._table([(P, None, 38, 61, 0, 0), (P, None, 38, 64, 0, 0)])
    assert run(frames=_vp(mixed)) == UNSUPPORTED                        # one block partition for all images
    assert run(pred=P + 2) == UNSUPPORTED and run(sums=P + 4) == UNSUPPORTED and run(partials=P + 4) == UNSUPPORTED
    assert run(frames=_vp(_frames(image=P + 1))) == UNSUPPORTED
    assert run(frames=_vp(mixed), sums=None) == BAD_ARG and run(pred=P + 2, n=0) == BAD_ARG
    # the single-frame entry point, now the launch of one image: its refusals as they were
    one = lib.ge_depth_metrics_resized
    assert one(None, 12, 20, P, 38, 61, 1e-3, 200.0, P, P, None) == BAD_ARG and one(P, 12, 20, P, 0, 61, 1e-3, 200.0, P, P, None) == BAD_ARG
    assert one(P, 12, 20, P + 2, 38, 61, 1e-3, 200.0, P, P, None) == UNSUPPORTED and one(P, 12, 20, P, 38, 61, 1e-3, 200.0, P + 4, P, None) == UNSUPPORTED


def test_wrappers_refuse_before_the_library():
    with pytest.raises(ValueError, match='1 .. 8'):
        DB.infer_front_ddad_batch([], [], torch.zeros(2, 5, 12, 20), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='2 frames and 1 ground depths'):
        DB.infer_front_ddad_batch([torch.zeros(38, 61, 3, dtype=torch.uint8)] * 2, [torch.zeros(38, 61)], torch.zeros(2, 5, 12, 20), (0, 0, 0),
                                  (1, 1, 1))
    with pytest.raises(ValueError, match='out must be'):
        DB.infer_front_ddad_batch([torch.zeros(38, 61, 3, dtype=torch.uint8)] * 2, [torch.zeros(38, 61)] * 2, torch.zeros(1, 5, 12, 20),
                                  (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match='MI355X only'):             # CPU tensors are not run
        DB.infer_front_ddad_batch([torch.zeros(38, 61, 3, dtype=torch.uint8)], [torch.zeros(38, 61)], torch.zeros(1, 5, 12, 20), (0, 0, 0),
                                  (1, 1, 1))
    sums = torch.zeros(9, 10, dtype=torch.float64)
    with pytest.raises(ValueError, match='1 .. 8'):
        DB.depth_metric_sums_resized_batch(torch.zeros(9, 12, 20), [torch.zeros(38, 61)] * 9, 1e-3, 200, sums)
    with pytest.raises(ValueError, match='pred must be'):
        DB.depth_metric_sums_resized_batch(torch.zeros(1, 12, 20), [torch.zeros(38, 61)] * 2, 1e-3, 200, sums)
    with pytest.raises(ValueError, match='ten float64'):
        DB.depth_metric_sums_resized_batch(torch.zeros(2, 12, 20), [torch.zeros(38, 61)] * 2, 1e-3, 200, sums[:1])
    with pytest.raises(RuntimeError, match='MI355X only'):
        DB.depth_metric_sums_resized_batch(torch.zeros(2, 12, 20), [torch.zeros(38, 61)] * 2, 1e-3, 200, sums)


# ------------------------------------------------------------------------------------------------ engine and loop, CPU models
def _cpu_model(cfg_name):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, cfg_name))
    cfg.model.pretrained = None
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.cfg = cfg
    return model.eval()


@pytest.fixture(scope='module')
def ddad_model():
    return _cpu_model('depthformer_v_ddad.py')


def test_batch_ddad_engine_argument_errors_before_device_work(ddad_model):
    """A CPU model: building the engine would raise something else (``torch.cuda.Stream``), so each error below comes before it; the
    per-batch errors are those of ``check_ddad_batch``, which ``batch`` runs before its first device call."""
    from gedepth_amd.depth import apis
    from gedepth_amd.depth.apis.batch_inference import BatchDDADInferencer, BatchDepthInferencer, check_batch, check_ddad_batch
    from gedepth_amd.depth.apis.inference import _config_of
    assert apis.BatchDDADInferencer is BatchDDADInferencer and 'BatchDDADInferencer' in apis.__all__
    for frames in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match=r'1 \.\. 8'):
            BatchDDADInferencer(ddad_model, frames)
    with pytest.raises(NotImplementedError, match='KITTI'):
        BatchDDADInferencer(_cpu_model('depthformer_swint_v.py'), 2)
    with pytest.raises(NotImplementedError, match='DDAD'):              # the KITTI engine keeps refusing a DDAD config
        BatchDepthInferencer(ddad_model, 2)
    spec = _config_of(ddad_model)[0]
    assert spec['protocol'] == 'ddad' and (spec['height'], spec['width']) == (384, 640)
    with pytest.raises(NotImplementedError, match='DDAD'):              # what inference_depther(batch > 1) asks
        check_batch(2, spec)
    assert check_batch(2, spec, 'eval_batch', ddad=True) == 2
    size = (1216, 1936)
    cams, taken = check_ddad_batch(spec, 4, [size] * 3, None, ['CAMERA_01', None, 'CAMERA_09'], [None, '/d/rgb/CAMERA_05/0.png', None])
    assert cams == ['CAMERA_01', 'CAMERA_05', 'CAMERA_09'] and taken == size
    with pytest.raises(ValueError, match='0 frames for an engine of 4 slots'):
        check_ddad_batch(spec, 4, [], None, None, None)
    with pytest.raises(ValueError, match='5 frames for an engine of 4 slots'):
        check_ddad_batch(spec, 4, [size] * 5, None, ['CAMERA_01'] * 5, None)
    with pytest.raises(ValueError, match='1 cameras for 2 frames'):
        check_ddad_batch(spec, 4, [size] * 2, None, ['CAMERA_01'], None)
    with pytest.raises(ValueError, match='3 ground depths for 2 frames'):
        check_ddad_batch(spec, 4, [size] * 2, [None] * 3, ['CAMERA_01'] * 2, None)
    with pytest.raises(ValueError, match='CAMERA_07'):                  # no known height
        check_ddad_batch(spec, 4, [size] * 2, None, ['CAMERA_01', 'CAMERA_07'], None)
    with pytest.raises(ValueError, match='no camera for frame 1'):
        check_ddad_batch(spec, 4, [size] * 2, None, ['CAMERA_01', None], [None, '/somewhere/0.png'])
    with pytest.raises(ValueError, match='smaller than DDADResize'):
        check_ddad_batch(spec, 4, [size, (300, 1936)], None, ['CAMERA_01'] * 2, None)
    with pytest.raises(ValueError, match=r'takes frames of \(1216, 1936\)'):
        check_ddad_batch(spec, 4, [size, (1216, 1940)], None, ['CAMERA_01'] * 2, None)
    with pytest.raises(ValueError, match=r'takes frames of \(1000, 1936\)'):
        check_ddad_batch(spec, 4, [size], None, ['CAMERA_01'], None, frame_size=(1000, 1936))


class _DDADLoader:
    """A loader whose dataset is a bare DDADDataset: the refusals below may touch no attribute of it."""
    batch_sampler = [[0], [1]]

    def __init__(self):
        from gedepth_amd.depth.datasets.ddad import DDADDataset
        self.dataset = DDADDataset.__new__(DDADDataset)


def test_eval_batch_with_ddad_argument_errors_before_device_work(ddad_model):
    from gedepth_amd.depth.apis.test import single_gpu_test
    from gedepth_amd.depth.core import ErrorMaps, StrataSpec
    loader = _DDADLoader()
    for bad in (0, 9):
        with pytest.raises(ValueError, match=r'eval_batch must be an integer in 1 \.\. 8'):
            single_gpu_test(ddad_model, loader, pre_eval=True, device_eval=True, eval_batch=bad)
    with pytest.raises(NotImplementedError, match='device_eval=True'):
        single_gpu_test(ddad_model, loader, pre_eval=True, eval_batch=2)
    with pytest.raises(NotImplementedError, match='ground_dir with eval_batch > 1'):
        single_gpu_test(ddad_model, loader, pre_eval=True, device_eval=True, eval_batch=2, ground_dir='d')
    with pytest.raises(NotImplementedError, match='pre_eval=True'):
        single_gpu_test(ddad_model, loader, device_eval=True, eval_batch=2)
    # strata and errors keep their refusals of the DDAD protocol, whatever eval_batch
    with pytest.raises(NotImplementedError, match='strata: DDADDataset is not evaluated by the KITTI protocol'):
        single_gpu_test(ddad_model, loader, pre_eval=True, device_eval=True, eval_batch=2, strata=StrataSpec())
    with pytest.raises(NotImplementedError, match='errors: DDADDataset is not evaluated by the KITTI protocol'):
        single_gpu_test(ddad_model, loader, pre_eval=True, device_eval=True, eval_batch=2, errors=ErrorMaps())
    # a KITTI model on the DDAD split: the protocol mismatch, as with eval_batch=1
    kitti = _cpu_model('depthformer_swint_v.py')
    with pytest.raises(NotImplementedError, match=r'DDADDataset.*ddad.*kitti'):
        single_gpu_test(kitti, loader, pre_eval=True, device_eval=True, eval_batch=2)


def test_ddad_dataset_batch_call_argument_errors(tmp_path):
    from gedepth_amd.depth.datasets.ddad import DDADDataset
    ds = DDADDataset.__new__(DDADDataset)
    np.savez_compressed(tmp_path / 'ok.npz', depth=np.arange(12, dtype=np.float64).reshape(3, 4))
    np.savez_compressed(tmp_path / 'bad.npz', depth=np.zeros((1, 3, 4), np.float32))
    ds.img_infos = [dict(ann=dict(depth_map=str(tmp_path / 'ok.npz'))), dict(ann=dict(depth_map=str(tmp_path / 'bad.npz')))]
    raw = ds.gt_raw(0)
    assert raw.dtype == np.float32 and raw.shape == (3, 4) and raw.flags.c_contiguous and raw[2, 3] == 11.0
    with pytest.raises(TypeError, match='2-D depth array'):
        ds.gt_raw(1)
    sums = torch.zeros(2, 10, dtype=torch.float64)
    with pytest.raises(TypeError, match='CUDA'):
        ds.pre_eval_device_batch(torch.zeros(2, 1, 12, 20), [0, 0], sums)          # a host tensor


# ------------------------------------------------------------------------------------------------ command lines
def _cli(name):
    spec = importlib.util.spec_from_file_location(f'tools_{name}_cli_ddad_batch', os.path.join(ROOT, 'tools', f'{name}.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_eval_batch_with_a_ddad_config():
    cli = _cli('test')
    cfg = os.path.join(CFG, 'depthformer_a_ddad.py')
    args = cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--device-eval', '--eval-batch', '4'])
    assert args.eval_batch == 4 and args.device_eval and cli.parse_args([cfg]).eval_batch == 1
    with pytest.raises(ValueError, match='--eval-batch needs --device-eval'):
        cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--eval-batch', '2'])
    with pytest.raises(ValueError, match='1 .. 8'):
        cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--device-eval', '--eval-batch', '9'])
    with pytest.raises(ValueError, match='--ground-dir'):
        cli.parse_args([cfg, '--eval', 'x', '--synthetic', '0', '--device-eval', '--eval-batch', '2', '--ground-dir', 'd'])


def test_benchmark_eval_builds_a_ddad_tree(tmp_path):
    """tools/benchmark_eval.py with a DDAD config: the synthetic tree at a small geometry — PNG frames, compressed ground truth with about
    1 % valid pixels, one ``ddad_pe.npz`` per camera for two cameras — read back through ``DDADDataset``."""
    from gedepth_amd.depth.datasets.ddad import DDADDataset
    from gedepth_amd.depth.datasets.pipelines import loading
    bench = _cli('benchmark_eval')
    split = bench.make_ddad_tree(str(tmp_path), frames=10, seed=1, unique=4, size=(40, 64))
    ds = DDADDataset(pipeline=[], split=split, test_mode=True, cameras=list(loading._DDAD_CAMERA_HEIGHT))
    assert len(ds) == 10
    cams = {ds.camera_of(i) for i in range(len(ds))}
    assert len(cams) >= 2 and cams <= set(loading._DDAD_CAMERA_HEIGHT)
    for cam in cams:
        assert np.load(os.path.join(str(tmp_path), 'pe', cam, 'ddad_pe.npz'))['pe'].shape == (40, 64)
    gt = ds.gt_raw(0)
    assert gt.shape == (40, 64) and 0 < (gt > 0).mean() < 0.05
    with open(ds.img_infos[0]['ann']['depth_map'], 'rb') as fh:         # np.savez_compressed: a deflated zip member
        assert fh.read(2) == b'PK' and int.from_bytes(fh.read(8)[6:8], 'little') == 8
    frame = ds.engine_frame(0)
    assert frame['img'].endswith('.png') and frame['camera'] in cams
