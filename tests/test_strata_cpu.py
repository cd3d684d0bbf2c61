"""Stratified device evaluation without a GPU: the fourth header table, the size queries and every argument refusal of
include/gedepth_strata.h (the library loads here and validates before it launches), the wrappers' and the loop's argument errors, the
host functions (``StrataSpec``, ``strata_table``, ``interleave_shards``), the ``--strata`` parser, and — from the numpy restatement alone —
what the inputs of tests/test_strata_gpu.py promise."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import strata_cases as SC
import strata_ref as SR
from gedepth_amd import batch_kernels as B
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = 10001, 10002
P = 4096                                                             # a fake non-null, 16-byte aligned pointer that is never followed


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


def _edges(*v):
    return (ctypes.c_float * len(v))(*v)


# ------------------------------------------------------------------------------------------------ header table
def test_fourth_header_is_parsed_and_bound():
    assert hip.STRATA_HEADERS == {'STRATA_SIGNATURES': 'gedepth_strata.h'}
    tables = {**hip.HEADERS, **hip.EXTRA_HEADERS, **hip.SCENE_HEADERS, **hip.STRATA_HEADERS}
    assert len(tables) == len(hip.HEADERS) + len(hip.EXTRA_HEADERS) + len(hip.SCENE_HEADERS) + 1
    header = open(os.path.join(ROOT, 'include', 'gedepth_strata.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.STRATA_SIGNATURES) == {'ge_depth_strata_count', 'ge_depth_metrics_strata_workspace', 'ge_depth_metrics_strata',
                                                      'ge_depth_metrics_strata_batch'}
    names = [set(getattr(hip, t)) for t in tables]
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            assert not names[a] & names[b], (list(tables)[a], list(tables)[b])
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.STRATA_SIGNATURES['ge_depth_strata_count'] == (i, [i, i])
    assert hip.STRATA_SIGNATURES['ge_depth_metrics_strata_workspace'] == (c.c_size_t, [i, i, i, i])
    assert hip.STRATA_SIGNATURES['ge_depth_metrics_strata'] == (i, [vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, f, f, vp, i, f, vp, vp, vp])
    assert hip.STRATA_SIGNATURES['ge_depth_metrics_strata_batch'] == (i, [vp, vp, i, i, i, i, i, i, i, f, f, f, vp, i, f, vp, vp, vp])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    for name, (res, args) in hip.STRATA_SIGNATURES.items():
        fn = getattr(hip.lib(), name)                                  # lib() has bound the fourth table too
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_kernels_reexports_by_an_import_line_only():
    from gedepth_amd import kernels
    from gedepth_amd import strata_kernels as K
    assert kernels.depth_metric_sums_strata is K.depth_metric_sums_strata
    assert kernels.depth_metric_sums_strata_batch is K.depth_metric_sums_strata_batch
    text = open(os.path.join(ROOT, 'gedepth_amd', 'kernels.py')).read()
    assert 'ge_depth_metrics_strata' not in text and 'ge_depth_strata_count' not in text


# ------------------------------------------------------------------------------------------------ size queries
def test_size_queries():
    lib = hip.lib()
    assert [lib.ge_depth_strata_count(n, 0) for n in range(-1, 9)] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0]
    assert [lib.ge_depth_strata_count(n, 1) for n in range(-1, 9)] == [0, 2, 4, 6, 8, 10, 12, 14, 16, 0]
    for Hc, Wc in ((352, 1216), (37, 515), (1, 1)):
        one = lib.ge_depth_metrics_workspace(Hc, Wc)
        assert one > 0
        for n in (1, 3, 8):
            for S in (1, 2, 8, 16):
                assert lib.ge_depth_metrics_strata_workspace(n, Hc, Wc, S) == n * S * one
    for n, Hc, Wc, S in ((0, 8, 24, 4), (9, 8, 24, 4), (-1, 8, 24, 4), (2, 0, 24, 4), (2, 8, 0, 4), (2, 8, -3, 4), (2, 8, 24, 0), (2, 8, 24, 17),
                         (2, 8, 24, -1)):
        assert lib.ge_depth_metrics_strata_workspace(n, Hc, Wc, S) == 0, (n, Hc, Wc, S)


# ------------------------------------------------------------------------------------------------ argument errors, no launch
def _single(pred=P, gt=P, ground=P, H=11, W=30, top=3, left=3, Hc=8, Wc=24, rect=(0, 8, 0, 24), edges='default', n_edges=3, tol=0.1,
            partials=P, sums=P):
    edges = _vp(_edges(20, 40, 60)) if isinstance(edges, str) else edges
    return hip.lib().ge_depth_metrics_strata(pred, gt, ground, H, W, top, left, Hc, Wc, *rect, 256.0, 1e-3, 80.0, edges, n_edges, tol, partials,
                                             sums, None)


def _frames(n=2, image=P, aux=P, H=11, W=30, top=3, left=3):
    return B._table([(image, aux, H, W, top, left)] * n)


def _batch(pred=P, frames='default', n=2, Hc=8, Wc=24, rect=(0, 8, 0, 24), edges='default', n_edges=3, tol=0.1, partials=P, sums=P):
    frames = _vp(_frames(n if 1 <= n <= 8 else 8)) if isinstance(frames, str) else frames
    edges = _vp(_edges(20, 40, 60)) if isinstance(edges, str) else edges
    return hip.lib().ge_depth_metrics_strata_batch(pred, frames, n, Hc, Wc, *rect, 256.0, 1e-3, 80.0, edges, n_edges, tol, partials, sums, None)


BAD_EDGES = {'descending': (40, 20, 60), 'equal': (20, 20, 60), 'nan': (20, float('nan'), 60), 'inf': (20, 40, float('inf')),
             '-inf': (float('-inf'), 40, 60)}


@pytest.mark.parametrize('run', [_single, _batch], ids=['single', 'batch'])
def test_shared_refusals(run):
    for name in ('pred', 'partials', 'sums'):
        assert run(**{name: None}) == BAD_ARG, name
    assert run(edges=None) == BAD_ARG                                  # n_edges = 3 without edges
    for n_edges in (-1, 8):
        assert run(n_edges=n_edges) == BAD_ARG, n_edges
    for what, e in BAD_EDGES.items():
        assert run(edges=_vp(_edges(*e))) == BAD_ARG, what
    for tol in (float('nan'), -0.01, 1.01, float('inf')):
        assert run(tol=tol) == BAD_ARG, tol
    for rect in ((-1, 8, 0, 24), (0, 9, 0, 24), (0, 8, -1, 24), (0, 8, 0, 25)):
        assert run(rect=rect) == BAD_ARG, rect
    assert run(Hc=0) == BAD_ARG and run(Wc=-4) == BAD_ARG
    for name in ('partials', 'sums'):
        assert run(**{name: P + 4}) == UNSUPPORTED, name
    # a bad argument wins over an unsupported one
    assert run(partials=P + 4, tol=2.0) == BAD_ARG


def test_single_image_refusals():
    assert _single(gt=None) == BAD_ARG
    assert _single(top=4) == BAD_ARG and _single(left=7) == BAD_ARG                      # the window leaves (H, W)
    assert _single(H=0) == BAD_ARG and _single(top=-1) == BAD_ARG
    assert _single(ground=P + 2) == UNSUPPORTED and _single(pred=P + 2) == UNSUPPORTED and _single(gt=P + 1) == UNSUPPORTED
    assert _single(ground=P + 2, n_edges=9) == BAD_ARG


def test_batch_refusals():
    assert _batch(frames=None) == BAD_ARG
    for n in (0, 9, -1):
        assert _batch(n=n) == BAD_ARG, n
    assert _batch(frames=_vp(_frames(image=None))) == BAD_ARG
    assert _batch(frames=_vp(_frames(top=4))) == BAD_ARG
    mixed = B._table([(P, P, 11, 30, 3, 3), (P, None, 11, 30, 3, 3)])
    assert _batch(frames=_vp(mixed)) == BAD_ARG                        # a ground plane for some frames only
    mixed = B._table([(P, None, 11, 30, 3, 3), (P, P, 11, 30, 3, 3), (P, None, 11, 30, 3, 3)])
    assert _batch(frames=_vp(mixed), n=3) == BAD_ARG
    assert _batch(frames=_vp(_frames(aux=P + 2))) == UNSUPPORTED
    assert _batch(Wc=22, rect=(0, 8, 0, 22)) == UNSUPPORTED and _batch(pred=P + 4) == UNSUPPORTED
    assert _batch(frames=_vp(_frames(image=P + 1))) == UNSUPPORTED


def test_wrapper_argument_errors():
    from gedepth_amd import kernels
    pred, raw = torch.zeros(8, 24), torch.zeros(11, 30, dtype=torch.uint16)
    ground, out = torch.zeros(11, 30), torch.zeros(8, 10, dtype=torch.float64)
    args = (pred, raw, 3, 3, (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(ValueError, match='0 .. 7'):
        kernels.depth_metric_sums_strata(*args, out, edges=range(1, 9), ground=ground)
    with pytest.raises(ValueError, match='strictly ascending'):
        kernels.depth_metric_sums_strata(*args, out, edges=(20, 20, 60), ground=ground)
    with pytest.raises(ValueError, match='ground_tol'):
        kernels.depth_metric_sums_strata(*args, out, edges=(20, 40, 60), ground=ground, ground_tol=1.5)
    with pytest.raises(ValueError, match='ground_tol'):
        kernels.depth_metric_sums_strata(*args, out, edges=(20, 40, 60), ground=ground, ground_tol=float('nan'))
    with pytest.raises(ValueError, match='8 strata'):
        kernels.depth_metric_sums_strata(*args, out[:4], edges=(20, 40, 60), ground=ground)
    with pytest.raises(ValueError, match='4 strata'):
        kernels.depth_metric_sums_strata(*args, out, edges=(20, 40, 60))                 # no ground: S = 4
    with pytest.raises(ValueError, match='shape'):
        kernels.depth_metric_sums_strata(*args, out, edges=(20, 40, 60), ground=ground[:, :29])
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums_strata(*args, out, edges=(20, 40, 60), ground=ground)  # host tensors
    preds, outs = torch.zeros(2, 8, 24), torch.zeros(2, 8, 10, dtype=torch.float64)
    bargs = (preds, [raw, raw], [3, 3], [3, 3], (0, 8, 0, 24), 256, 1e-3, 80)
    with pytest.raises(ValueError, match='1 .. 8'):
        kernels.depth_metric_sums_strata_batch(preds, [], [], [], (0, 8, 0, 24), 256, 1e-3, 80, outs)
    with pytest.raises(ValueError, match='grounds'):
        kernels.depth_metric_sums_strata_batch(*bargs, outs, edges=(20, 40, 60), grounds=[ground, None])
    with pytest.raises(ValueError, match='grounds'):
        kernels.depth_metric_sums_strata_batch(*bargs, outs, edges=(20, 40, 60), grounds=[ground])
    with pytest.raises(ValueError, match='8 strata'):
        kernels.depth_metric_sums_strata_batch(*bargs, outs[:, :4], edges=(20, 40, 60), grounds=[ground, ground])
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_metric_sums_strata_batch(*bargs, outs, edges=(20, 40, 60), grounds=[ground, ground])


def test_loop_argument_errors_on_a_cpu_model():
    from gedepth_amd.depth.apis.test import multi_gpu_test, single_gpu_test
    from gedepth_amd.depth.core import StrataSpec
    from gedepth_amd.depth.datasets.ddad import DDADDataset
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    model = torch.nn.Linear(1, 1)

    class Loader:
        dataset = KITTIDataset.__new__(KITTIDataset)
        batch_sampler = [[0]]
    with pytest.raises(NotImplementedError, match='device_eval'):
        single_gpu_test(model, Loader(), pre_eval=True, strata=StrataSpec())
    with pytest.raises(NotImplementedError, match='device_eval'):
        multi_gpu_test(model, Loader(), pre_eval=True, strata=StrataSpec())

    class DDADLoader:
        dataset = DDADDataset.__new__(DDADDataset)
        batch_sampler = [[0]]
    with pytest.raises(NotImplementedError, match='DDADDataset.*KITTI protocol'):
        single_gpu_test(model, DDADLoader(), pre_eval=True, device_eval=True, strata=StrataSpec())
    ds = KITTIDataset.__new__(KITTIDataset)
    with pytest.raises(TypeError, match='CUDA'):
        ds.pre_eval_device_strata(torch.zeros(1, 352, 1216), 0, None, StrataSpec(), None)
    with pytest.raises(TypeError, match='CUDA'):
        ds.pre_eval_device_strata_batch(torch.zeros(2, 1, 352, 1216), [0, 1], None, StrataSpec(), None)


def test_ground_class_without_a_ground_depth_is_refused():
    from gedepth_amd.depth.apis.test import _strata_ground
    from gedepth_amd.depth.core import StrataSpec

    class Engine:                                                      # every engine answers to the one name
        last_ground_depths = None
    with pytest.raises(NotImplementedError, match='ground depth'):
        _strata_ground(Engine(), StrataSpec())
    assert _strata_ground(Engine(), StrataSpec(ground=False)) is None


# ------------------------------------------------------------------------------------------------ host functions
def test_strata_spec_names_and_count():
    from gedepth_amd.depth import core
    from gedepth_amd.depth.core import StrataSpec
    assert core.StrataSpec is StrataSpec and 'StrataSpec' in core.__all__ and 'strata_table' in core.__all__
    spec = StrataSpec()
    assert (spec.edges, spec.ground, spec.ground_tol, spec.count) == ((20.0, 40.0, 60.0), True, 0.1, 8)
    assert spec.names(1e-3, 80) == ['0-20m/other', '0-20m/ground', '20-40m/other', '20-40m/ground', '40-60m/other', '40-60m/ground',
                                    '60-80m/other', '60-80m/ground']
    bins = StrataSpec((10, 30.5), ground=False)
    assert bins.count == 3 and bins.names(1e-3, 80) == ['0-10m', '10-30.5m', '30.5-80m']
    assert StrataSpec((), ground=False).count == 1 and StrataSpec((), ground=False).names(1e-3, 80) == ['0-80m']
    assert StrataSpec(range(1, 8)).count == 16
    for s in (spec, bins):
        assert s.count == hip.lib().ge_depth_strata_count(len(s.edges), int(s.ground))
    for bad in (dict(edges=range(8)), dict(edges=(20, 20)), dict(edges=(40, 20)), dict(edges=(float('nan'),)), dict(edges=(float('inf'),)),
                dict(ground_tol=-0.1), dict(ground_tol=1.1), dict(ground_tol=float('nan'))):
        with pytest.raises(ValueError):
            StrataSpec(**bad)


def _row(gt, pred):
    import eval_ref as R
    return R.sums_f64(np.asarray(gt, np.float32), np.asarray(pred, np.float32))


def test_strata_table_on_hand_made_rows():
    from gedepth_amd.depth.core import StrataSpec, metrics_from_sums, strata_table
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    spec = StrataSpec((20,), ground=True)                              # S = 4
    zero = np.zeros(10)
    a0, a1 = _row([5, 10, 15], [5.5, 9, 30]), _row([8], [8.8])         # stratum 0 in both images
    b0 = _row([30, 50], [33, 20])                                      # stratum 2 in image 0 only
    rows = np.array([[a0, zero, b0, zero], [a1, zero, zero, zero]])    # stratum 1 and 3: empty everywhere
    table = strata_table(rows, spec, 1e-3, 80)
    assert list(table) == spec.names(1e-3, 80) == ['0-20m/other', '0-20m/ground', '20-80m/other', '20-80m/ground']
    for entry in table.values():
        assert list(entry) == list(METRIC_NAMES) + ['pixels', 'images']
    m0, m1 = metrics_from_sums(a0), metrics_from_sums(a1)
    for k, name in enumerate(METRIC_NAMES):
        assert table['0-20m/other'][name] == pytest.approx((m0[k] + m1[k]) / 2, rel=1e-15)      # the mean over images, not over pixels
        assert table['20-80m/other'][name] == pytest.approx(metrics_from_sums(b0)[k], rel=1e-15)   # image 1 is skipped, not counted as 0
        assert np.isnan(table['0-20m/ground'][name]) and np.isnan(table['20-80m/ground'][name])
    assert [e['images'] for e in table.values()] == [2, 0, 1, 0]
    assert [e['pixels'] for e in table.values()] == [4 / 6, 0.0, 2 / 6, 0.0]
    assert sum(e['pixels'] for e in table.values()) == pytest.approx(1.0, abs=1e-15)
    with pytest.raises(ValueError, match=r'\(N, 4, 10\)'):
        strata_table(rows[:, :3], spec)
    empty = strata_table(np.zeros((2, 4, 10)), spec)
    assert all(np.isnan(e['pixels']) and e['images'] == 0 for e in empty.values())


def test_evaluate_strata_prints_and_flattens():
    from gedepth_amd.depth.core import StrataSpec
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    ds = KITTIDataset.__new__(KITTIDataset)
    ds.min_depth, ds.max_depth = 1e-3, 80
    spec = StrataSpec((20,), ground=False)
    rows = np.array([[_row([5, 10], [5.5, 9]), _row([30], [33])]])
    lines = []

    class Logger:
        info = staticmethod(lines.append)
    flat = ds.evaluate_strata(rows, spec, logger=Logger())
    assert len(flat) == 2 * 11 and flat['0-20m.pixels'] == 2 / 3 and flat['20-80m.images'] == 1 and flat['20-80m.abs_rel'] == pytest.approx(0.1)
    assert len(lines) == 1 and lines[0].startswith('Strata:') and '0-20m' in lines[0] and 'abs_rel' in lines[0]


def test_interleave_shards_on_lists_and_arrays():
    from gedepth_amd.depth.apis.test import interleave_shards
    assert interleave_shards([[0, 3, 6], [1, 4, 7], [2, 5, 8]], 9) == list(range(9))
    assert interleave_shards([[0, 2, 4], [1, 3, 0]], 5) == [0, 1, 2, 3, 4]                # the sampler padded the last round
    assert interleave_shards([['a'], []], 1) == ['a']
    rows = np.arange(7 * 2 * 10, dtype=np.float64).reshape(7, 2, 10)
    shards = [rows[0::3], rows[1::3], rows[2::3]]                       # 3 + 2 + 2
    out = interleave_shards(shards, 7)
    assert isinstance(out, np.ndarray) and out.shape == (7, 2, 10) and np.array_equal(out, rows)
    padded = [np.concatenate([rows[0::2]]), np.concatenate([rows[1::2], rows[:1]])]      # 4 + 4, one padded
    assert np.array_equal(interleave_shards(padded, 7), rows)


# ------------------------------------------------------------------------------------------------ parser
def _tool():
    spec = importlib.util.spec_from_file_location('tools_test_for_strata', os.path.join(ROOT, 'tools', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_strata_options_and_their_clashes():
    T = _tool()
    base = ['cfg.py', '--eval', 'x', '--device-eval', '--synthetic', '0']
    args = T.parse_args(base)
    assert args.strata is None and T.strata_spec(args) is None
    args = T.parse_args(base + ['--strata'])
    spec = T.strata_spec(args)
    assert args.strata == [20.0, 40.0, 60.0] and (spec.edges, spec.ground, spec.ground_tol) == ((20.0, 40.0, 60.0), True, 0.1)
    args = T.parse_args(base + ['--strata', '10', '25.5', '--strata-ground-tol', '0.05', '--strata-no-ground', '--strata-out', 'o/s.npz',
                                '--eval-batch', '4'])
    spec = T.strata_spec(args)
    assert (spec.edges, spec.ground, spec.ground_tol, args.strata_out, args.eval_batch) == ((10.0, 25.5), False, 0.05, 'o/s.npz', 4)
    for bad, match in ((['cfg.py', '--strata'], 'needs --eval and --device-eval'),
                       (['cfg.py', '--eval', 'x', '--strata', '20'], 'needs --eval and --device-eval'),
                       (base + ['--strata-out', 's.npz'], 'need --strata'),
                       (base + ['--strata-no-ground'], 'need --strata'),
                       (base + ['--strata', '--strata-out', 's.pkl'], '.npz'),
                       (['cfg.py', '--scene-dir', 'd', '--strata'], 'needs --eval and --device-eval')):
        with pytest.raises(ValueError, match=match):
            T.parse_args(bad)
    with pytest.raises(ValueError, match='strictly ascending'):
        T.strata_spec(T.parse_args(base + ['--strata', '40', '20']))


# ------------------------------------------------------------------------------------------------ what the GPU inputs promise
@pytest.mark.parametrize('name', list(SC.CASES))
def test_case_populates_and_empties_the_designated_strata(name):
    c = SC.CASES[name]
    assert c['S'] == SR.count(c['edges'], c['ground']) == hip.lib().ge_depth_strata_count(len(c['edges']), int(c['ground'] is not None))
    assert c['populated'] | c['empty'] == set(range(c['S'])) and not c['populated'] & c['empty']
    _, mask, stratum = SR.window_strata(c['raw'], c['ground'], c['geom'], c['rect'], c['edges'], c['tol'])
    counts = [int((stratum == s).sum()) for s in range(c['S'])]
    assert sum(counts) == int(mask.sum()) and int((stratum == -1).sum()) == mask.size - int(mask.sum())
    assert {s for s, n in enumerate(counts) if n} == c['populated'], counts
    assert {s for s, n in enumerate(counts) if not n} == c['empty'], counts
    sums = SR.strata_sums(c['raw'], c['pred'], c['ground'], c['geom'], c['rect'], c['edges'], c['tol'])
    assert sums.shape == (c['S'], 10) and [int(v) for v in sums[:, 0]] == counts


@pytest.mark.parametrize('name', [n for n, c in SC.CASES.items() if c['boundary'] and c['geom'][:2] != (1, 1)])
def test_case_holds_the_boundary_pixels(name):
    c = SC.CASES[name]
    top, left = c['geom'][2:4]
    gt, mask, stratum = SR.window_strata(c['raw'], c['ground'], c['geom'], c['rect'], c['edges'], c['tol'])
    C = 2 if c['ground'] is not None else 1
    pos = SC.boundary_positions(c['rect'])
    assert len(set(pos)) == 16 and all(mask[p] for p in pos), 'every boundary pixel counts'
    edges = c['edges'][:3]
    if edges:
        assert edges == SC.EDGES
        for k, e in enumerate(edges):                                    # on the edge: the upper bin; one raw step below: the lower one
            assert gt[pos[k]] == np.float32(e) and stratum[pos[k]] // C == k + 1, (k, e)
            assert gt[pos[3 + k]] == np.float32(e) - np.float32(1 / 256) and stratum[pos[3 + k]] // C == k, (k, e)
    if c['ground'] is None:
        return
    g = c['ground'][top:top + c['geom'][4], left:left + c['geom'][5]]
    tol = np.float32(c['tol'])
    assert c['tol'] == 0.125
    on = {p: bool(stratum[p] % 2) for p in pos}
    for k in (6, 7):                                                     # |gt - g| == tol * g exactly: on the ground
        assert g[pos[k]] == 16 and np.abs(gt[pos[k]] - g[pos[k]]) == tol * g[pos[k]] == 2 and on[pos[k]], k
    assert (gt[pos[6]], gt[pos[7]]) == (14, 18) and (int(c['raw'][top + pos[6][0], left + pos[6][1]]), int(c['raw'][top + pos[7][0], left + pos[7][1]])) == (3584, 4608)
    ulp = np.spacing(np.float32(16))
    assert g[pos[8]] == g[pos[10]] == np.float32(16) + ulp and g[pos[9]] == g[pos[11]] == np.float32(16) - ulp / 2      # the neighbours of 16
    assert [on[pos[k]] for k in (8, 9, 10, 11)] == [False, True, True, False]
    for k in (8, 9, 10, 11):                                             # one ulp of g moves the pixel across the boundary, by less than 2 ulp
        diff = float(np.abs(gt[pos[k]] - g[pos[k]])) - float(tol * g[pos[k]])
        assert 0 < abs(diff) <= 2 * float(ulp) and (diff <= 0) == on[pos[k]], (k, diff)
    vals = [g[pos[k]] for k in (12, 13, 14, 15)]
    assert vals[0] == 0 and vals[1] < 0 and np.isnan(vals[2]) and np.isposinf(vals[3])
    assert [on[pos[k]] for k in (12, 13, 14)] == [False, False, False]   # no plane, and NaN: off the ground
    assert on[pos[15]]                                                   # +inf: inf <= inf, as the header's expression reads


def test_cases_cover_both_ground_load_paths():
    vec = SC.CASES['vector-edge-beyond-max']
    H, W, top, left, Hc, Wc = vec['geom']
    assert W % 4 == 0 and left % 4 == 0 and Wc % 4 == 0 and vec['ground_offset'] == 0
    assert SC.CASES['vector-ground-odd-offset']['geom'] == vec['geom'] and SC.CASES['vector-ground-odd-offset']['ground_offset'] == 1
    assert SC.CASES['odd-left-scalar']['geom'][3] % 2 == 1
