"""Error images and split-level error planes without a GPU: the sixth header table, every argument refusal of include/gedepth_error.h (the
library loads here and validates before it launches), the wrappers', the engine's and the loop's argument errors, the host functions
(``error_bands``, ``ERROR_COLOURS``, ``ErrorMaps``), the ``--error-dir`` parser, and — from the numpy restatement alone — what the inputs
of tests/test_error_gpu.py promise.

The last group (``test_case_holds_what_the_gpu_test_needs``, ``test_cases_cover_the_load_and_store_paths``,
``test_accumulate_restatement_is_a_sequential_float64_sum``) checks the fixtures and the restatement, not the library: apart from the one
comparison with ``depth.utils.error_bands`` these tests would pass without the feature.  They are here so that a GPU test that fails can
be read as the kernel's fault and not the inputs'."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import error_cases as EC
import error_ref as ER
from gedepth_amd import batch_kernels as B
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = 10001, 10002
P = 4096                                                             # a fake non-null, 16-byte aligned pointer that is never followed
ENTRY_POINTS = {'ge_error_image', 'ge_error_image_batch', 'ge_error_accumulate', 'ge_error_accumulate_batch'}


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ header table
def test_error_header_is_parsed_and_every_symbol_is_exported():
    assert hip.ERROR_HEADERS == {'ERROR_SIGNATURES': 'gedepth_error.h'}
    header = open(os.path.join(ROOT, 'include', 'gedepth_error.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.ERROR_SIGNATURES) == ENTRY_POINTS
    others = {**hip.HEADERS, **hip.EXTRA_HEADERS, **hip.SCENE_HEADERS, **hip.STRATA_HEADERS, **hip.NECK_HEADERS}
    for table in others:
        assert not set(getattr(hip, table)) & ENTRY_POINTS, table
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.ERROR_SIGNATURES['ge_error_image'] == (i, [vp, vp, vp] + [i] * 10 + [f, f, f, f, i, i, vp, vp, vp])
    assert hip.ERROR_SIGNATURES['ge_error_image_batch'] == (i, [vp, vp] + [i] * 7 + [f, f, f, f, i, i, vp, vp, vp])
    assert hip.ERROR_SIGNATURES['ge_error_accumulate'] == (i, [vp, vp] + [i] * 10 + [f, f, f, vp, vp, vp])
    assert hip.ERROR_SIGNATURES['ge_error_accumulate_batch'] == (i, [vp, vp] + [i] * 7 + [f, f, f, vp, vp, vp])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name, (res, args) in hip.ERROR_SIGNATURES.items():
        assert hasattr(raw, name), f'{name} is declared in the header and not exported by the library'
        fn = getattr(hip.lib(), name)                                  # lib() has bound the sixth table too
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_kernels_reexports_by_an_import_line_only():
    from gedepth_amd import error_kernels as K
    from gedepth_amd import kernels
    for name in ('error_image', 'error_image_batch', 'error_accumulate', 'error_accumulate_batch'):
        assert getattr(kernels, name) is getattr(K, name)
    text = open(os.path.join(ROOT, 'gedepth_amd', 'kernels.py')).read()
    assert 'ge_error_' not in text
    assert (K.MAX_RADIUS, K.BACKGROUNDS) == (3, (0, 1, 2))


# ------------------------------------------------------------------------------------------------ the band rule
def test_band_rule_on_every_threshold():
    from gedepth_amd.depth.utils import ERROR_COLOURS, error_bands
    c = EC.threshold_case()
    tau = np.float32(EC.THRESHOLD_TAU)
    gt = c['raw'].astype(np.float32) / np.float32(256)
    assert (gt == 16).all()
    pred = c['pred'][0]
    n = (np.abs(gt[0] - pred) / gt[0]) / tau                           # float32 throughout
    assert n.dtype == np.float32
    want, below = [], 0
    for j, t in enumerate(ER.T):
        for side in range(2):
            k = 4 * j + 2 * side
            assert n[k] == np.float32(t), (j, side, n[k])              # exactly on the threshold: the upper band
            assert np.float32(t) * np.float32(0.999) < n[k + 1] <= np.float32(t), (j, side, n[k + 1])
            below += int(n[k + 1] < np.float32(t))                     # (16 - the smallest denormal is 16 again: that neighbour stays on T = 16)
            want += [j + 1, j if n[k + 1] < np.float32(t) else j + 1]
    assert below == 17
    assert list(ER.bands(n)) == want
    assert list(error_bands(n)) == want and error_bands(n).dtype == np.uint8
    picture, err = ER.error_image(c['raw'], c['pred'], c['frame'], c['geom'], c['rect'], EC.THRESHOLD_TAU, 0, 2)
    assert np.array_equal(picture[0], ER.BGR[want]) and np.array_equal(err[0] / tau, n)
    assert np.array_equal(ERROR_COLOURS[:, ::-1], ER.BGR) and ERROR_COLOURS.dtype == np.uint8 and ERROR_COLOURS.shape == (10, 3)
    assert tuple(ERROR_COLOURS[0]) == (49, 54, 149) and tuple(ERROR_COLOURS[9]) == (165, 0, 38)


def test_error_bands_agrees_with_the_restatement():
    from gedepth_amd.depth.utils import error_bands
    rng = np.random.default_rng(0)
    n = np.concatenate([np.exp2(rng.uniform(-8, 8, 4000)).astype(np.float32), np.array(ER.T, np.float32),
                        np.nextafter(np.array(ER.T, np.float32), np.float32(0)), np.float32([0, np.inf, np.nan, 1e30, 1e-30, -0.0])])
    got = error_bands(n.reshape(2, -1))
    assert got.shape == (2, n.size // 2) and np.array_equal(got.ravel(), ER.bands(n))
    assert list(error_bands(np.float32([0, np.inf, np.nan, 15.999, 16]))) == [0, 9, 9, 8, 9]
    assert set(got.ravel()) == set(range(10))


# ------------------------------------------------------------------------------------------------ ErrorMaps
def test_error_maps_argument_errors():
    from gedepth_amd.depth import core
    from gedepth_amd.depth.core import ErrorMaps
    assert core.ErrorMaps is ErrorMaps and 'ErrorMaps' in core.__all__ and 'StrataSpec' in core.__all__
    e = ErrorMaps()
    assert (e.out_dir, e.tau, e.radius, e.background, e.frames, e.sum, e.count) == (None, 0.05, 1, 1, 0, None, None)
    e = ErrorMaps('d', 1.0, 3, 2)
    assert (e.out_dir, e.tau, e.radius, e.background) == ('d', 1.0, 3, 2)
    for bad in (dict(tau=0), dict(tau=-0.1), dict(tau=1.01), dict(tau=float('nan')), dict(tau='x'), dict(radius=-1), dict(radius=4),
                dict(radius=1.5), dict(radius=True), dict(background=3), dict(background=-1), dict(background=0.0)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ErrorMaps(**bad)
    with pytest.raises(TypeError, match='out_dir'):
        ErrorMaps(out_dir=3)
    for call in (e.mean, e.rows, lambda: e.save('nowhere')):
        with pytest.raises(RuntimeError, match='no planes'):
            call()


def test_error_maps_mean_rows_and_save(tmp_path):
    from PIL import Image
    from gedepth_amd.depth.core import ErrorMaps
    e = ErrorMaps(tau=0.0625)
    e.sum, e.count, e.rect, e.frames = np.zeros((352, 1216)), np.zeros((352, 1216), np.uint32), (143, 349, 43, 1172), 3
    e.sum[200, 100], e.count[200, 100] = 0.0625 * 3, 3                   # mean 0.0625: n == 1, band 5
    e.sum[201, 7], e.count[201, 7] = 0.5, 1                              # n == 8: band 8
    e.sum[351, 1215], e.count[351, 1215] = 0.001, 2                      # n == 0.008: band 0
    mean = e.mean()
    assert mean[200, 100] == 0.0625 and mean[201, 7] == 0.5 and np.isnan(mean[0, 0]) and int(np.isfinite(mean).sum()) == 3
    m, c = e.rows(8)
    assert m.shape == c.shape == (44,) and c[25] == 4 and m[25] == (0.0625 * 3 + 0.5) / 4 and c[43] == 2 and np.isnan(m[0]) and c.sum() == 6
    m1, c1 = e.rows()
    assert m1.shape == (352,) and c1[200] == 3 and c1[201] == 1
    with pytest.raises(ValueError, match='step'):
        e.rows(0)
    out = str(tmp_path / 'errors')
    e.save(out)
    z = np.load(os.path.join(out, 'summary.npz'))
    assert np.array_equal(z['sum'], e.sum) and np.array_equal(z['count'], e.count) and z['count'].dtype == np.uint32 and z['sum'].dtype == np.float64
    assert float(z['tau']) == 0.0625 and tuple(z['rect']) == e.rect and int(z['frames']) == 3
    rgb = np.asarray(Image.open(os.path.join(out, 'mean_abs_rel.png')))
    assert rgb.shape == (352, 1216, 3)
    assert tuple(rgb[200, 100]) == ER.RGB[5] and tuple(rgb[201, 7]) == ER.RGB[8] and tuple(rgb[351, 1215]) == ER.RGB[0]
    assert int((rgb != 0).any(-1).sum()) == 3                            # black where nothing was counted
    other = ErrorMaps()
    other.sum, other.count, other.frames = e.sum.copy(), e.count.copy(), 3
    other.add(e.sum, e.count, 3)
    assert other.frames == 6 and other.count[200, 100] == 6 and other.count.dtype == np.uint32 and other.sum[201, 7] == 1.0


# ------------------------------------------------------------------------------------------------ the C entry points: no launch
def _image(pred=P, gt=P, image=P, H=11, W=30, top=3, left=3, Hc=8, Wc=24, rect=(0, 8, 0, 24), tau=0.05, radius=1, background=1, out=P, err=P):
    return hip.lib().ge_error_image(pred, gt, image, H, W, top, left, Hc, Wc, *rect, 256.0, 1e-3, 80.0, tau, radius, background, out, err, None)


def _frames(n=2, image=P, aux=P, H=11, W=30, top=3, left=3):
    return B._table([(image, aux, H, W, top, left)] * n)


def _image_batch(pred=P, frames='default', n=2, Hc=8, Wc=24, rect=(0, 8, 0, 24), tau=0.05, radius=1, background=1, out=P, err=P):
    frames = _vp(_frames(n if 1 <= n <= 8 else 8)) if isinstance(frames, str) else frames
    return hip.lib().ge_error_image_batch(pred, frames, n, Hc, Wc, *rect, 256.0, 1e-3, 80.0, tau, radius, background, out, err, None)


def _acc(pred=P, gt=P, H=11, W=30, top=3, left=3, Hc=8, Wc=24, rect=(0, 8, 0, 24), sum=P, count=P):
    return hip.lib().ge_error_accumulate(pred, gt, H, W, top, left, Hc, Wc, *rect, 256.0, 1e-3, 80.0, sum, count, None)


def _acc_batch(pred=P, frames='default', n=2, Hc=8, Wc=24, rect=(0, 8, 0, 24), sum=P, count=P):
    frames = _vp(_frames(n if 1 <= n <= 8 else 8)) if isinstance(frames, str) else frames
    return hip.lib().ge_error_accumulate_batch(pred, frames, n, Hc, Wc, *rect, 256.0, 1e-3, 80.0, sum, count, None)


@pytest.mark.parametrize('run', [_image, _image_batch, _acc, _acc_batch], ids=['image', 'image-batch', 'accumulate', 'accumulate-batch'])
def test_shared_refusals(run):
    assert run(pred=None) == BAD_ARG
    for rect in ((-1, 8, 0, 24), (0, 9, 0, 24), (0, 8, -1, 24), (0, 8, 0, 25)):
        assert run(rect=rect) == BAD_ARG, rect
    assert run(Hc=0) == BAD_ARG and run(Wc=-4) == BAD_ARG


@pytest.mark.parametrize('run', [_image, _image_batch], ids=['single', 'batch'])
def test_image_refusals(run):
    assert run(out=None) == BAD_ARG                                    # (a null err is allowed: it would launch, so it is not tried here)
    for radius in (-1, 4):
        assert run(radius=radius) == BAD_ARG, radius
    for background in (-1, 3):
        assert run(background=background) == BAD_ARG, background
    for tau in (float('nan'), 0.0, -0.05, 1.0001, float('inf')):
        assert run(tau=tau) == BAD_ARG, tau
    assert run(err=P + 2) == UNSUPPORTED
    assert run(err=P + 2, radius=9) == BAD_ARG                         # a bad argument wins over an unsupported one


def test_single_image_refusals():
    assert _image(gt=None) == BAD_ARG
    assert _image(image=None) == BAD_ARG and _image(image=None, background=0) == BAD_ARG     # a null frame only with background 2
    assert _image(top=4) == BAD_ARG and _image(left=7) == BAD_ARG                            # the window leaves (H, W)
    assert _image(H=0) == BAD_ARG and _image(top=-1) == BAD_ARG
    assert _image(pred=P + 2) == UNSUPPORTED and _image(gt=P + 1) == UNSUPPORTED
    assert _acc(gt=None) == BAD_ARG and _acc(sum=None) == BAD_ARG and _acc(count=None) == BAD_ARG
    assert _acc(top=4) == BAD_ARG and _acc(left=7) == BAD_ARG
    assert _acc(sum=P + 4) == UNSUPPORTED and _acc(count=P + 2) == UNSUPPORTED and _acc(pred=P + 2) == UNSUPPORTED and _acc(gt=P + 1) == UNSUPPORTED
    assert _acc(sum=P + 4, rect=(0, 9, 0, 24)) == BAD_ARG


def test_batch_refusals():
    for run in (_image_batch, _acc_batch):
        assert run(frames=None) == BAD_ARG
        for n in (0, 9, -1):
            assert run(n=n) == BAD_ARG, n
        assert run(frames=_vp(_frames(image=None))) == BAD_ARG
        assert run(frames=_vp(_frames(top=4))) == BAD_ARG
        assert run(Wc=22, rect=(0, 8, 0, 22)) == UNSUPPORTED and run(pred=P + 4) == UNSUPPORTED
        assert run(frames=_vp(_frames(image=P + 1))) == UNSUPPORTED
    mixed = B._table([(P, P, 11, 30, 3, 3), (P, None, 11, 30, 3, 3)])
    for background in (0, 1):
        assert _image_batch(frames=_vp(mixed), background=background) == BAD_ARG             # a frame for some images only
        assert _image_batch(frames=_vp(_frames(aux=None)), background=background) == BAD_ARG
    assert _acc_batch(sum=None) == BAD_ARG and _acc_batch(count=None) == BAD_ARG
    assert _acc_batch(sum=P + 4) == UNSUPPORTED and _acc_batch(count=P + 2) == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ wrappers, engine, loop
def test_wrapper_argument_errors():
    from gedepth_amd import kernels
    pred, raw, frame = torch.zeros(8, 24), torch.zeros(11, 30, dtype=torch.uint16), torch.zeros(11, 30, 3, dtype=torch.uint8)
    args = (pred, raw, frame, 3, 3, (0, 8, 0, 24), 256, 1e-3, 80)
    for kw, match in ((dict(tau=0), 'tau'), (dict(tau=float('nan')), 'tau'), (dict(tau=1.5), 'tau'), (dict(radius=4), 'radius'),
                      (dict(radius=0.5), 'radius'), (dict(background=3), 'background')):
        with pytest.raises(ValueError, match=match):
            kernels.error_image(*args, **kw)
        with pytest.raises(ValueError, match=match):
            kernels.error_image_batch(pred[None], [raw], [frame], [3], [3], (0, 8, 0, 24), 256, 1e-3, 80, **kw)
    with pytest.raises(ValueError, match='background=2'):
        kernels.error_image(pred, raw, None, 3, 3, (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(ValueError, match='leaves'):
        kernels.error_image(pred, raw, frame, 4, 3, (0, 8, 0, 24), 256, 1e-3, 80)           # the window leaves the frame
    with pytest.raises(ValueError, match='rectangle'):
        kernels.error_image(pred, raw, frame, 3, 3, (0, 9, 0, 24), 256, 1e-3, 80)
    with pytest.raises(ValueError, match=r'\(H, W, 3\)'):
        kernels.error_image(pred, raw, frame[:, :29], 3, 3, (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(TypeError, match='numpy arrays throughout'):
        kernels.error_image(pred.numpy(), raw, frame, 3, 3, (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.error_image(*args)                                                           # host tensors
    with pytest.raises(ValueError, match='1 .. 8'):
        kernels.error_image_batch(pred[None], [], [], [], [], (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(ValueError, match='background=2'):
        kernels.error_image_batch(pred[None].repeat(2, 1, 1), [raw, raw], [frame, None], [3, 3], [3, 3], (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.error_image_batch(pred[None], [raw], [frame], [3], [3], (0, 8, 0, 24), 256, 1e-3, 80)
    s, n = torch.zeros(8, 24, dtype=torch.float64), torch.zeros(8, 24, dtype=torch.int32).view(torch.uint32)
    with pytest.raises(ValueError, match='planes'):
        kernels.error_accumulate(pred, raw, 3, 3, (0, 8, 0, 24), 256, 1e-3, 80, s[:4], n)
    with pytest.raises(ValueError, match='leaves'):
        kernels.error_accumulate(pred, raw, 3, 7, (0, 8, 0, 24), 256, 1e-3, 80, s, n)
    with pytest.raises(TypeError, match='float64'):
        kernels.error_accumulate(pred.numpy(), raw.numpy(), 3, 3, (0, 8, 0, 24), 256, 1e-3, 80, np.zeros((8, 24), np.float32), np.zeros((8, 24), np.uint32))
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.error_accumulate(pred, raw, 3, 3, (0, 8, 0, 24), 256, 1e-3, 80, s, n)
    with pytest.raises(ValueError, match='1 .. 8'):
        kernels.error_accumulate_batch(pred[None], [], [], [], (0, 8, 0, 24), 256, 1e-3, 80, s, n)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.error_accumulate_batch(pred[None], [raw], [3], [3], (0, 8, 0, 24), 256, 1e-3, 80, s, n)


def test_engines_refuse_before_any_device_work():
    from gedepth_amd.depth.apis.batch_inference import BatchDepthInferencer
    from gedepth_amd.depth.apis.inference import DepthInferencer
    ddad = DepthInferencer.__new__(DepthInferencer)
    ddad.ddad = True
    with pytest.raises(NotImplementedError, match='KITTI protocol'):
        ddad.error_map('frame.png', 'gt.png')
    kitti = DepthInferencer.__new__(DepthInferencer)
    kitti.ddad, kitti.spec = False, dict(height=352, width=1216)
    for kw, match in ((dict(tau=0), 'tau'), (dict(radius=7), 'radius'), (dict(background=5), 'background'), (dict(rect=(0, 353, 0, 1216)), 'rect')):
        with pytest.raises(ValueError, match=match):
            kitti.error_map('frame.png', 'gt.png', **kw)
    batch = BatchDepthInferencer.__new__(BatchDepthInferencer)
    with pytest.raises(NotImplementedError, match='error_map'):
        batch.error_map('frame.png', 'gt.png')
    from gedepth_amd.depth import apis
    assert 'inference_error_map' in apis.__all__ and callable(apis.inference_error_map)
    with pytest.raises(ValueError, match='gt='):
        apis.inference_error_map(torch.nn.Linear(1, 1), 'frame.png', None)


def test_loop_argument_errors_on_a_cpu_model():
    from gedepth_amd.depth.apis.test import multi_gpu_test, single_gpu_test
    from gedepth_amd.depth.core import ErrorMaps
    from gedepth_amd.depth.datasets.ddad import DDADDataset
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    model = torch.nn.Linear(1, 1)

    class Loader:
        dataset = KITTIDataset.__new__(KITTIDataset)
        batch_sampler = [[0]]
    with pytest.raises(NotImplementedError, match='device_eval'):
        single_gpu_test(model, Loader(), pre_eval=True, errors=ErrorMaps())
    with pytest.raises(NotImplementedError, match='device_eval'):
        multi_gpu_test(model, Loader(), pre_eval=True, errors=ErrorMaps())
    with pytest.raises(NotImplementedError, match='device_eval'):
        single_gpu_test(model, Loader(), scene_dir='d', errors=ErrorMaps())                  # checked before scene_dir's own refusal
    with pytest.raises(NotImplementedError, match='scene_dir with .*errors'):
        single_gpu_test(model, Loader(), scene_dir='d', device_eval=True, errors=ErrorMaps())

    class DDADLoader:
        dataset = DDADDataset.__new__(DDADDataset)
        batch_sampler = [[0]]
    with pytest.raises(NotImplementedError, match='DDADDataset.*KITTI protocol'):
        single_gpu_test(model, DDADLoader(), pre_eval=True, device_eval=True, errors=ErrorMaps())
    ds = KITTIDataset.__new__(KITTIDataset)
    with pytest.raises(TypeError, match='CUDA'):
        ds.pre_eval_device_errors(torch.zeros(1, 352, 1216), 0, ErrorMaps(), None)
    with pytest.raises(TypeError, match='CUDA'):
        ds.pre_eval_device_errors_batch(torch.zeros(2, 1, 352, 1216), [0, 1], ErrorMaps(), None)


def test_padded_shards_stay_out_of_the_planes():
    """A non-shuffled DistributedSampler pads the last round with the split's first entries; ``_unpadded`` counts a rank's own."""
    from torch.utils.data import DistributedSampler
    from gedepth_amd.depth.apis.test import _unpadded, interleave_shards
    for total, world in ((4, 3), (652, 8), (7, 2), (8, 4), (5, 8), (1, 1)):
        kept = []
        for rank in range(world):
            shard = list(DistributedSampler(range(total), num_replicas=world, rank=rank, shuffle=False))
            real = _unpadded(len(shard), total, rank, world)
            assert 0 <= real <= len(shard) and len(shard) - real <= -(-total // world), (total, world, rank)
            kept.append(shard[:real])
        flat = interleave_shards(kept, total)
        assert flat == list(range(total)), (total, world)             # every image once: no padded duplicate among the kept ones
    assert sum(_unpadded(82, 652, r, 8) for r in range(8)) == 652 and _unpadded(82, 652, 4, 8) == 81 and _unpadded(82, 652, 3, 8) == 82
    ds = __import__('gedepth_amd.depth.datasets.kitti', fromlist=['KITTIDataset']).KITTIDataset
    from gedepth_amd.depth.core import ErrorMaps
    with pytest.raises(TypeError, match='CUDA'):                        # the count keyword exists and the refusals still come first
        ds.__new__(ds).pre_eval_device_errors_batch(torch.zeros(2, 1, 352, 1216), [0, 1], ErrorMaps(), None, count=1)


# ------------------------------------------------------------------------------------------------ parser
def _tool():
    spec = importlib.util.spec_from_file_location('tools_test_for_errors', os.path.join(ROOT, 'tools', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_error_options_and_their_clashes():
    T = _tool()
    base = ['cfg.py', '--eval', 'x', '--device-eval', '--synthetic', '0']
    args = T.parse_args(base)
    assert args.error_dir is None and T.error_maps(args) is None
    e = T.error_maps(T.parse_args(base + ['--error-dir', 'd']))
    assert (e.out_dir, e.tau, e.radius, e.background) == ('d', 0.05, 1, 1)
    args = T.parse_args(base + ['--error-dir', 'd', '--error-tau', '0.1', '--error-radius', '3', '--error-no-pictures', '--eval-batch', '4',
                                '--strata'])
    e = T.error_maps(args)
    assert (e.out_dir, e.tau, e.radius, args.error_dir, args.eval_batch) == (None, 0.1, 3, 'd', 4) and T.strata_spec(args) is not None
    for bad, match in ((['cfg.py', '--error-dir', 'd'], 'needs --eval and --device-eval'),
                       (['cfg.py', '--eval', 'x', '--error-dir', 'd'], 'needs --eval and --device-eval'),
                       (base + ['--error-tau', '0.1'], 'need --error-dir'),
                       (base + ['--error-radius', '2'], 'need --error-dir'),
                       (base + ['--error-no-pictures'], 'need --error-dir'),
                       (base + ['--error-dir', 'd', '--error-tau', '0'], r'\(0, 1\]'),
                       (base + ['--error-dir', 'd', '--error-tau', '2'], r'\(0, 1\]'),
                       (base + ['--error-dir', 'd', '--error-radius', '4'], '0 .. 3'),
                       (['cfg.py', '--scene-dir', 's', '--error-dir', 'd'], '--scene-dir cannot be combined with --error-dir')):
        with pytest.raises(ValueError, match=match):
            T.parse_args(bad)


# ------------------------------------------------------------------------------------------------ what the GPU inputs promise
@pytest.mark.parametrize('name', list(EC.CASES))
def test_case_holds_what_the_gpu_test_needs(name):
    c = EC.CASES[name]
    H, W, top, left, Hc, Wc = c['geom']
    r0, r1, c0, c1 = c['rect']
    gt, mask = ER.counted(c['raw'], c['geom'], c['rect'], c['limits'])
    err = ER.error_plane(c['raw'], c['pred'], c['geom'], c['rect'], c['limits'])
    assert (err[~mask] == -1).all() and mask.sum() > 30
    inside = np.zeros(mask.shape, bool)
    inside[r0:r1, c0:c1] = True
    placed = set(c['placed'])
    if not inside.all():                                                # (one case counts the whole crop: its corners paint instead)
        outside = [p for p in placed if gt[p] > 0 and not inside[p]]
        assert len(outside) >= 4 and not mask[tuple(zip(*outside))].any(), 'returns just outside the rectangle, not counted'
    row = r0 + 1                                                        # raw 0, at and next to min_depth, at and next to max_depth, 65535
    assert [bool(mask[row, c0 + 2 + 2 * k]) for k in range(6)] == [False, False, True, False, True, False]
    assert gt[row, c0 + 4] == np.float32(c['limits'][1]) or name != 'width-35'                # gt == min_depth exactly where 1 / 256 is the limit
    assert gt[row, c0 + 8] == 80
    odd = [c['pred'][r1 - 2, c0 + 2 + 3 * k] for k in range(5)]
    assert np.isnan(odd[0]) and np.isposinf(odd[1]) and odd[2] == 0 and odd[3] < 0 and np.isneginf(odd[4])
    assert all(mask[r1 - 2, c0 + 2 + 3 * k] for k in range(5))
    e = err[r1 - 2, c0 + 2:c0 + 15:3]
    assert np.isnan(e[0]) and np.isposinf(e[1]) and e[2] == 1 and e[3] > 1 and np.isposinf(e[4])
    for radius in (0, 1, 3):
        picture, plane = EC.expected(name, radius, 1)
        assert np.array_equal(plane, err, equal_nan=True)
        colours = {tuple(px) for px in picture[_dilated(mask, radius)]}
        assert colours == {tuple(b) for b in ER.BGR}, 'every band 0 .. 9 occurs'
        back = ~_dilated(mask, radius)
        window = c['frame'][top:top + Hc, left:left + Wc]
        assert back.any() and np.array_equal(picture[back], window[back] >> 1)
        assert np.array_equal(EC.expected(name, radius, 0)[0][back], window[back]) and not EC.expected(name, radius, 2)[0][back].any()
    from gedepth_amd.depth.utils import ERROR_COLOURS, error_bands       # the library's numpy band rule paints the undilated picture
    with np.errstate(all='ignore'):
        n = err[mask] / np.float32(EC.TAU)
    assert np.array_equal(EC.expected(name, 0, 2)[0][mask], ERROR_COLOURS[error_bands(n)][:, ::-1])
    rm, cm = (r0 + r1) // 2, (c0 + c1) // 2
    lone = EC.expected(name, 1, 2)[0][rm - 2:rm + 3, cm - 10:cm - 5]                          # the isolated return: a 3 x 3 square
    assert (lone.any(-1)).sum() == 9 and lone[1:4, 1:4].any(-1).all()
    pair = EC.expected(name, 1, 2)[0][rm, cm + 11:cm + 15]                                    # 0.01 and 0.5 side by side: the larger wins
    small, large = (tuple(ER.BGR[ER.bands(np.float32([v / EC.TAU]))[0]]) for v in (0.01, 0.5))
    assert [tuple(p) for p in pair] == [small, large, large, large]                          # where both reach, also on the smaller one's own pixel
    assert tuple(EC.expected(name, 0, 2)[0][rm, cm + 12]) == tuple(ER.BGR[ER.bands(np.float32([0.01 / EC.TAU]))[0]])


def _dilated(mask, radius):
    out = np.zeros(mask.shape, bool)
    for r, c in zip(*np.nonzero(mask)):
        out[max(r - radius, 0):r + radius + 1, max(c - radius, 0):c + radius + 1] = True
    return out


def test_cases_cover_the_load_and_store_paths():
    a, b, v, w = (EC.CASES[n]['geom'] for n in ('one-tile-odd-left', 'tiles-and-remainders', 'tiles-garg-aligned', 'width-35'))
    assert a == (23, 50, 6, 7, 17, 36) and a[3] % 2 == 1 and EC.CASES['one-tile-odd-left']['rect'] == (2, 15, 3, 33)
    assert b == (75, 270, 5, 3, 70, 264) and b[4] > 64 and b[5] > 256                         # two tiles and a remainder up to 64 x 256 tiles
    assert v[1] % 4 == 0 and v[3] % 4 == 0 and v[5] % 4 == 0
    assert w[5] == 35 and EC.BATCHABLE == ['one-tile-odd-left', 'tiles-and-remainders', 'tiles-garg-aligned']
    placed = set(EC.CASES['tiles-and-remainders']['placed'])
    rows, cols = {p[0] for p in placed}, {p[1] for p in placed}
    assert all(s - 1 in rows and s in rows for s in EC.SEAM_ROWS) and all(s - 1 in cols and s in cols for s in EC.SEAM_COLS)
    assert {(0, 0), (0, 263), (69, 0), (69, 263)} <= placed
    mask = ER.counted(EC.CASES['tiles-and-remainders']['raw'], b, (0, 70, 0, 264))[1]
    assert mask[0, 0] and mask[0, 263] and mask[69, 0] and mask[69, 263]                      # the corners count where the rectangle is the crop


def test_accumulate_restatement_is_a_sequential_float64_sum():
    c = EC.CASES['one-tile-odd-left']
    frames = [(c['raw'], c['pred']), (c['raw'], c['pred'] * np.float32(1.01)), (c['raw'], c['pred'])]
    shape = c['geom'][4:]
    s0, n0 = np.full(shape, 0.25), np.full(shape, 7, np.uint32)
    s, n = ER.accumulate(frames, [c['geom']] * 3, c['rect'], shape, s0, n0)
    e = [ER.error_plane(r, p, c['geom'], c['rect']) for r, p in frames]
    mask = ER.counted(c['raw'], c['geom'], c['rect'])[1]
    fin = [mask & np.isfinite(x) for x in e]
    want = s0.copy()
    for x, f in zip(e, fin):
        want[f] = want[f] + x[f].astype(np.float64)
    assert np.array_equal(s, want) and np.array_equal(n, n0 + sum(f.astype(np.uint32) for f in fin)) and n.dtype == np.uint32
    assert (s[~mask] == 0.25).all() and (n[~mask] == 7).all()
    never = mask & ~fin[0] & ~fin[1]
    assert never.sum() >= 3 and (s[never] == 0.25).all() and (n[never] == 7).all()            # NaN and inf enter neither plane
