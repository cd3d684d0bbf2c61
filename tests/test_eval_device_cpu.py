"""Device evaluation, the parts that need no GPU: the second header and its binding, argument validation of ``ge_depth_metrics``,
``metrics_from_sums`` against a float64 restatement of ``calculate``, and ``KITTIDataset.eval_rect`` against ``eval_mask``."""
import ctypes
import os
import re

import numpy as np
import pytest

import eval_ref as R
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 10001


def test_eval_header_parses_and_library_exports_it():
    header = open(os.path.join(ROOT, 'include', 'gedepth_eval.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.EVAL_SIGNATURES) == {'ge_depth_metrics', 'ge_depth_metrics_workspace'}
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.EVAL_SIGNATURES['ge_depth_metrics'] == (i, [vp, vp] + [i] * 10 + [f] * 3 + [vp, vp, vp])
    assert hip.EVAL_SIGNATURES['ge_depth_metrics_workspace'] == (c.c_size_t, [i, i])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    for name, (res, args) in hip.EVAL_SIGNATURES.items():            # lib() has bound the second table too
        fn = getattr(hip.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_training_header_is_unchanged_by_the_eval_entry_points():
    header = open(os.path.join(ROOT, 'include', 'gedepth_hip.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', header))
    assert declared == set(hip.SIGNATURES)
    assert not set(hip.SIGNATURES) & set(hip.EVAL_SIGNATURES)
    assert hip.lib().ge_abi_version() == 7


def test_argument_validation_without_a_gpu():
    """Every check comes before a launch, so fake non-null pointers are never followed."""
    lib = hip.lib()
    p = 4096                                                          # any aligned non-null address

    def run(pred=p, gt=p, H=11, W=27, top=3, left=3, Hc=8, Wc=20, rect=(0, 8, 0, 20), partials=p, sums=p):
        return lib.ge_depth_metrics(pred, gt, H, W, top, left, Hc, Wc, *rect, 256.0, 1e-3, 80.0, partials, sums, None)
    for null in ('pred', 'gt', 'partials', 'sums'):
        assert run(**{null: None}) == BAD_ARG, null
    for size in ('H', 'W', 'Hc', 'Wc'):
        assert run(**{size: 0}) == BAD_ARG and run(**{size: -4}) == BAD_ARG, size
    assert run(top=4) == BAD_ARG and run(left=8) == BAD_ARG          # 4 + 8 > 11, 8 + 20 > 27: the window leaves the frame
    assert run(top=-1) == BAD_ARG and run(left=-1) == BAD_ARG
    assert run(H=2 ** 31 - 1, top=2 ** 31 - 8) == BAD_ARG            # no overflow in top + Hc
    for rect in ((-1, 8, 0, 20), (0, 9, 0, 20), (0, 8, -1, 20), (0, 8, 0, 21), (9, 8, 0, 20), (0, 8, 21, 20)):
        assert run(rect=rect) == BAD_ARG, rect
    assert lib.ge_depth_metrics_workspace(0, 5) == 0 and lib.ge_depth_metrics_workspace(5, -1) == 0
    ws = lib.ge_depth_metrics_workspace(352, 1216)
    assert ws > 0 and ws % 80 == 0
    assert lib.ge_depth_metrics_workspace(1, 1) == 80


def test_depth_metric_sums_refuses_cpu_tensors():
    import torch
    from gedepth_amd import kernels
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums(torch.zeros(8, 20), torch.zeros(11, 27, dtype=torch.uint16), 3, 3, (0, 8, 0, 20), 256, 1e-3, 80,
                                  torch.zeros(10, dtype=torch.float64))


def _pixels(seed, n):
    rng = np.random.default_rng(seed)
    gt = (rng.integers(300, 20000, n).astype(np.float32) / np.float32(256))
    pred = (gt * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    return gt, pred


@pytest.mark.parametrize('n', [1, 2, 1000, 50001])
def test_metrics_from_sums_equals_float64_calculate(n):
    from gedepth_amd.depth.core import metrics_from_sums
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    gt, pred = _pixels(n, n)
    got = metrics_from_sums(R.sums_f64(gt, pred))
    ref = R.calculate_f64(gt, pred)
    assert len(got) == len(ref) == len(METRIC_NAMES) == 9
    for name, a, b in zip(METRIC_NAMES, got, ref):
        assert abs(a - b) <= 1e-12 * abs(b), (name, a, b)
    if n == 1:
        assert got[7] == 0                   # one pixel: the variance is 0 or a rounding-sized negative number -> NaN -> 0


def test_metrics_from_sums_edge_rows():
    from gedepth_amd.depth.core import metrics_from_sums
    empty = metrics_from_sums(np.zeros(10))
    assert len(empty) == 9 and all(np.isnan(v) for v in empty)
    # one pixel whose l^2 / n - (l / n)^2 rounds below zero: NaN under the square root becomes 0, as in calculate
    one = metrics_from_sums(np.array([1, 1, 1, 1, 0.1, 0.2, 4.0, 0.1, 0.1 * 0.1 * (1 - 1e-16), 0.05]))
    assert one[7] == 0 and one[4] == 2.0 and one[:3] == (1.0, 1.0, 1.0)
    nan_row = metrics_from_sums(np.array([2, 0, 0, 0, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan]))
    assert nan_row[:3] == (0.0, 0.0, 0.0) and np.isnan(nan_row[3]) and nan_row[7] == 0


@pytest.mark.parametrize('crop', ['garg', 'eigen', 'none'])
@pytest.mark.parametrize('shape', [(352, 1216), (8, 20)])
def test_eval_rect_is_the_bounding_box_of_eval_mask(crop, shape):
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    ds = KITTIDataset.__new__(KITTIDataset)
    ds.garg_crop, ds.eigen_crop, ds.min_depth, ds.max_depth = crop == 'garg', crop == 'eigen', 1e-3, 80
    mask = ds.eval_mask(np.full((1,) + shape, 10.0, np.float32))[0]            # every depth valid: the mask is the crop
    rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    r0, r1, c0, c1 = ds.eval_rect(*shape)
    assert (r0, r1, c0, c1) == (rows[0], rows[-1] + 1, cols[0], cols[-1] + 1)
    assert mask[r0:r1, c0:c1].all() and mask.sum() == (r1 - r0) * (c1 - c0)
    if crop == 'none':
        assert (r0, r1, c0, c1) == (0, shape[0], 0, shape[1])


def test_cli_flag_needs_eval_and_the_dataset_route(monkeypatch):
    import importlib.util
    monkeypatch.setenv('LOCAL_RANK', '0')
    spec = importlib.util.spec_from_file_location('ge_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(['cfg.py', '--eval', 'abs_rel', '--synthetic', '0', '--device-eval'])
    assert args.device_eval and not tool.parse_args(['cfg.py', '--eval', 'abs_rel', '--synthetic', '0']).device_eval
    for bad in (['--device-eval', '--synthetic', '0'], ['--device-eval', '--eval', 'x'], ['--device-eval', '--eval', 'x', '--synthetic', '0', '--show-dir', 'd']):
        with pytest.raises(ValueError, match='--device-eval'):
            tool.parse_args(['cfg.py'] + bad)
