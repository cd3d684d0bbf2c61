"""The prior sweep, the parts that need no GPU: the perturbation rule (tests/sweep_ref.py) against the model's own slope expression, the
baseline's pass-through, ``PriorSweep``, the ninth header table and its binding, the argument validation of ``ge_infer_front_sweep``
(every check comes before the launch), ``KITTIDataset.evaluate_sweep`` on hand-made rows, and every refusal of the loops, of
``inference_prior_sweep`` and of ``tools/test.py --prior-sweep``, raised before any device work."""
import ctypes
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import sweep_ref as R
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
BAD_ARG, UNSUPPORTED = 10001, 10002
P = 4096                                                             # a fake non-null, 16-byte aligned pointer that is never followed


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ the rule
def test_rule_agrees_with_the_models_slope_expression():
    """pe uniform in [1, 200], 41 pitches in [-5, 5] degrees: the rule and -h / ((-h / (pe + 1e-8)) - tan(slope) + 1e-8), both in numpy
    float32, within 1e-5 relative wherever q = 1 / pe + c >= 0.01 (measured: 1.4e-6)."""
    pe = np.random.default_rng(0).uniform(1.0, 200.0, 20000).astype(np.float32)
    worst, checked = 0.0, 0
    for d in np.linspace(-5.0, 5.0, 41):
        c = R.variant_c(d)
        got = R.perturb(pe, c, 1.0, False)
        ref = R.model_plane(pe, d)
        q = np.float32(1) / pe + c
        keep = q >= np.float32(0.01)
        rel = np.abs(got[keep].astype(np.float64) - ref[keep]) / np.abs(ref[keep].astype(np.float64))
        worst, checked = max(worst, float(rel.max())), checked + int(keep.sum())
    print(f'rule vs the model\'s expression: largest relative difference {worst:.2e} over {checked} draws')
    assert checked > 0.5 * 41 * pe.size and worst <= 1e-5              # the negative pitches push the far half of the plane below q = 0.01


def test_baseline_hands_its_input_through_bit_for_bit():
    pe = np.array([0.5, 3.0, 77.7, 300.0, 0.0, -0.0, -5.0, np.nan, np.inf, -np.inf, 1e-30, 3e38], np.float32)
    pe[7] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]                   # a NaN with a payload
    got = R.perturb(pe, 0.0, 1.0, False)
    np.testing.assert_array_equal(got.view(np.uint32), pe.view(np.uint32))
    # the formula at c = 0 would not: 1 / (1 / pe) is not pe in float32 (the reason for the branch)
    draws = np.random.default_rng(1).uniform(1.0, 200.0, 20000).astype(np.float32)
    assert (np.float32(1) / (np.float32(1) / draws) != draws).mean() > 0.05
    # the other branches: drop zeroes everything; not (pe > 0) stays whatever c and s are
    assert not R.perturb(pe, 0.01, 2.0, True).view(np.uint32).any()
    moved = R.perturb(pe, 0.01, 2.0, False)
    still = ~(pe > 0)
    np.testing.assert_array_equal(moved[still].view(np.uint32), pe[still].view(np.uint32))
    assert moved[8] == np.float32(2.0) / np.float32(0.01)                                      # +inf: q = c
    assert R.perturb(pe, -0.5, 1.0, False)[3] == 0.0                                            # q = 1 / 300 - 0.5 <= 0 -> 0


# ------------------------------------------------------------------------------------------------ PriorSweep
def test_prior_sweep_order_names_and_table():
    from gedepth_amd.depth.core import PriorSweep
    from gedepth_amd.depth.core.evaluation import PriorSweep as same
    assert PriorSweep is same
    spec = PriorSweep()
    assert spec.count == 6 == len(spec.variants) == len(spec.names)
    assert spec.names == ['baseline', 'pitch -1.00 deg', 'pitch -0.50 deg', 'pitch +0.50 deg', 'pitch +1.00 deg', 'no prior']
    table = spec.table()
    assert table[0] == (0.0, 1.0, 0) and table[-1] == (0.0, 1.0, 1)
    for row, d in zip(table[1:5], (-1.0, -0.5, 0.5, 1.0)):
        c = np.float32(np.tan(np.radians(d)) / 1.65)
        assert row == (float(c), 1.0, 0) and np.float32(row[0]) == c and isinstance(row[0], float) and isinstance(row[2], int)
    spec = PriorSweep(pitch_deg=(0.5,), height_scale=(0.95, 1.05), drop=False, cam_height=1.5)
    assert spec.names == ['baseline', 'pitch +0.50 deg', 'height x0.95', 'height x1.05'] and spec.count == 4
    assert spec.table() == [(0.0, 1.0, 0), (float(np.float32(np.tan(np.radians(0.5)) / 1.5)), 1.0, 0), (0.0, float(np.float32(0.95)), 0),
                            (0.0, float(np.float32(1.05)), 0)]
    assert PriorSweep(pitch_deg=(), drop=False).table() == [(0.0, 1.0, 0)]                      # the baseline is always there, once
    assert PriorSweep(pitch_deg=(-10.0, 10.0), height_scale=(0.5, 2.0)).count == 6             # the ranges' ends are allowed
    assert PriorSweep(pitch_deg=(-3, -2, -1, 1, 2, 3)).count == 8                               # the most there can be


@pytest.mark.parametrize('kw', [dict(pitch_deg=(-3, -2, -1, 1, 2, 3, 4)),                       # 9 variants
                                dict(pitch_deg=(1, 2, 3, 4), height_scale=(0.9, 1.1, 1.2)),      # 9 variants
                                dict(pitch_deg=(10.5,)), dict(pitch_deg=(-11.0,)), dict(pitch_deg=(float('nan'),)),
                                dict(pitch_deg=(float('inf'),)), dict(pitch_deg=(0.0,)),
                                dict(height_scale=(0.49,)), dict(height_scale=(2.01,)), dict(height_scale=(1.0,)),
                                dict(height_scale=(float('nan'),)),
                                dict(pitch_deg=(0.5, 0.5)), dict(height_scale=(1.1, 1.1)),
                                dict(cam_height=0.0), dict(cam_height=-1.65), dict(cam_height=float('nan'))],
                         ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_prior_sweep_value_errors(kw):
    from gedepth_amd.depth.core import PriorSweep
    with pytest.raises(ValueError, match='PriorSweep'):
        PriorSweep(**kw)


# ------------------------------------------------------------------------------------------------ the header table, the struct, the ABI
def test_sweep_header_is_parsed_and_bound():
    from gedepth_amd import kernels
    from gedepth_amd import sweep_kernels as S
    assert hip.SWEEP_HEADERS == {'SWEEP_SIGNATURES': 'gedepth_sweep.h'}
    header = open(os.path.join(ROOT, 'include', 'gedepth_sweep.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.SWEEP_SIGNATURES) == {'ge_infer_front_sweep', 'ge_prior_variant_size'}
    for table in ('SIGNATURES', 'EVAL_SIGNATURES', 'DDAD_SIGNATURES', 'CLOUD_SIGNATURES', 'GROUND_SIGNATURES', 'BATCH_SIGNATURES',
                  'SCENE_SIGNATURES', 'STRATA_SIGNATURES', 'NECK_SIGNATURES', 'ERROR_SIGNATURES', 'ACCUM_SIGNATURES', 'DDAD_BATCH_SIGNATURES'):
        assert not set(hip.SWEEP_SIGNATURES) & set(getattr(hip, table)), table
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.SWEEP_SIGNATURES['ge_infer_front_sweep'] == (i, [vp, vp, i, i, i, i, vp, i, vp, i, i, i, f, vp, vp, f, i, vp])
    assert hip.SWEEP_SIGNATURES['ge_prior_variant_size'] == (c.c_size_t, [])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    for name, (res, args) in hip.SWEEP_SIGNATURES.items():
        fn = getattr(hip.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert hip.lib().ge_abi_version() == 7 and len(hip.SIGNATURES) == 102                      # the versioned ABI has not moved
    assert ctypes.sizeof(S.GePriorVariant) == hip.lib().ge_prior_variant_size() == 12
    assert [n for n, _ in S.GePriorVariant._fields_] == ['c', 's', 'drop'] and S.SWEEP_MAX == 8
    assert kernels.infer_front_sweep is S.infer_front_sweep
    t = S.variant_table([(0.0, 1.0, 0), (0.25, 0.5, False), (0.0, 1.0, True)])
    assert [(v.c, v.s, v.drop) for v in t] == [(0.0, 1.0, 0), (0.25, 0.5, 0), (0.0, 1.0, 1)]


def _variants(rows=((0.0, 1.0, 0), (0.01, 1.0, 0))):
    from gedepth_amd.sweep_kernels import GePriorVariant
    return (GePriorVariant * len(rows))(*[GePriorVariant(*r) for r in rows])


def test_front_sweep_argument_validation_without_a_gpu():
    lib = hip.lib()
    m = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    eight = ((0.0, 1.0, 0),) * 8

    def run(bgr=P, pe=P, H=11, W=30, top=3, left=3, variants='default', n=2, dst=P, Hc=8, Wc=24, views=2, mean=m, std=m):
        variants = _vp(_variants(eight)) if variants == 'default' else variants
        return lib.ge_infer_front_sweep(bgr, pe, H, W, top, left, variants, n, dst, Hc, Wc, views, 200.0, _vp(mean) if mean else None,
                                        _vp(std) if std else None, 200.0, 1, None)
    for name in ('bgr', 'pe', 'variants', 'dst', 'mean', 'std'):
        assert run(**{name: None}) == BAD_ARG, name
    for n in (0, -1, 9):
        assert run(n=n) == BAD_ARG, n
    for views in (0, 3):
        assert run(views=views) == BAD_ARG
    assert run(H=0) == BAD_ARG and run(W=-30) == BAD_ARG and run(Hc=0) == BAD_ARG and run(Wc=-4) == BAD_ARG
    assert run(top=4) == BAD_ARG and run(left=7) == BAD_ARG and run(top=-1) == BAD_ARG and run(left=-1) == BAD_ARG     # 4 + 8 > 11, 7 + 24 > 30
    good = (0.0, 1.0, 0)
    for bad in ((float('nan'), 1.0, 0), (float('inf'), 1.0, 0), (0.0, float('nan'), 0), (0.0, float('inf'), 0), (0.0, 0.0, 0),
                (0.0, -1.0, 0), (float('nan'), 1.0, 1)):
        assert run(variants=_vp(_variants((good, bad))), n=2) == BAD_ARG, bad
    # a bad entry beyond n is not looked at; an unsupported layout comes after every bad argument
    assert run(variants=_vp(_variants((good, (float('nan'), 1.0, 0)))), n=1, Wc=22) == UNSUPPORTED
    assert run(Wc=22) == UNSUPPORTED and run(dst=P + 4) == UNSUPPORTED and run(pe=P + 2) == UNSUPPORTED
    assert run(Wc=22, n=9) == BAD_ARG and run(dst=P + 4, variants=_vp(_variants((good, (0.0, 0.0, 0))))) == BAD_ARG


def test_wrapper_refuses_before_the_library():
    from gedepth_amd import sweep_kernels as S
    bgr, pe, out = torch.zeros(11, 30, 3, dtype=torch.uint8), torch.zeros(11, 30), torch.zeros(4, 5, 8, 24)
    with pytest.raises(ValueError, match='1 .. 8'):
        S.infer_front_sweep(bgr, pe, [], out, 3, 3, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='1 .. 8'):
        S.infer_front_sweep(bgr, pe, [(0.0, 1.0, 0)] * 9, out, 3, 3, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='finite'):
        S.infer_front_sweep(bgr, pe, [(float('nan'), 1.0, 0)], out, 3, 3, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='s > 0'):
        S.infer_front_sweep(bgr, pe, [(0.0, 0.0, 0)], out, 3, 3, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='views'):
        S.infer_front_sweep(bgr, pe, [(0.0, 1.0, 0)] * 3, out, 3, 3, (0, 0, 0), (1, 1, 1))     # 6 images into 4
    with pytest.raises(RuntimeError, match='MI355X only'):                                     # CPU tensors are not run
        S.infer_front_sweep(bgr, pe, [(0.0, 1.0, 0)], out, 3, 3, (0, 0, 0), (1, 1, 1))


# ------------------------------------------------------------------------------------------------ evaluate_sweep
def test_evaluate_sweep_on_hand_made_rows():
    from gedepth_amd.depth.core import PriorSweep, metrics_from_sums
    from gedepth_amd.depth.core.evaluation import METRIC_NAMES
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    spec = PriorSweep(pitch_deg=(0.5,), drop=True)                    # baseline, pitch, no prior
    rng = np.random.default_rng(5)
    rows = np.zeros((3, 3, 10))
    for i in range(2):                                                # images 0 and 1 count pixels; image 2 counts none (n == 0)
        for v in range(3):
            n = 100.0 + 10 * i
            counts = np.sort(rng.integers(40, 100, 3)).astype(np.float64)
            rows[i, v] = [n, *counts, *rng.uniform(1.0, 50.0, 2), rng.uniform(100.0, 900.0), rng.uniform(-5.0, 5.0), rng.uniform(30.0, 60.0),
                          rng.uniform(1.0, 9.0)]
    ds = object.__new__(KITTIDataset)
    lines = []
    table = ds.evaluate_sweep(rows, spec, logger=types.SimpleNamespace(info=lines.append))
    assert list(table) == spec.names
    for v, name in enumerate(spec.names):
        tuples = [metrics_from_sums(rows[i, v]) for i in range(3)]
        assert all(np.isnan(t).all() for t in tuples[2:])             # the empty image is a NaN tuple and leaves the nan-mean
        for k, key in enumerate(METRIC_NAMES):
            assert table[name][key] == pytest.approx(np.mean([tuples[0][k], tuples[1][k]]), rel=1e-12), (name, key)
    assert not any(k.startswith('d_') for k in table['baseline'])
    for name in spec.names[1:]:
        for key in ('abs_rel', 'rmse', 'a1'):
            assert table[name][f'd_{key}'] == table[name][key] - table['baseline'][key]
    text = lines[0].split('\n')
    assert len(lines) == 1 and len(text) == 2 + 3 and text[0] == 'Prior sweep:' and [t.split(' | ')[0].strip() for t in text[2:]] == spec.names
    with pytest.raises(ValueError, match='evaluate_sweep'):
        ds.evaluate_sweep(rows[:, :2], spec)
    empty = ds.evaluate_sweep(np.zeros((0, 3, 10)), spec, logger=types.SimpleNamespace(info=lambda m: None))
    assert all(np.isnan(v) for v in empty['baseline'].values())


# ------------------------------------------------------------------------------------------------ refusals, before any device work
def _cpu_model(cfg_name):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, cfg_name))
    cfg.model.pretrained = None
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.cfg = cfg
    return model.eval()


def test_loop_refusals_before_the_first_frame():
    """``torch.nn.Identity()`` and no loader: anything past the refusals would raise something else."""
    from gedepth_amd.depth.apis.test import multi_gpu_test, single_gpu_test
    from gedepth_amd.depth.core import ErrorMaps, PriorSweep, StrataSpec
    spec, model = PriorSweep(), torch.nn.Identity()
    with pytest.raises(NotImplementedError, match='device_eval=True'):
        single_gpu_test(model, None, pre_eval=True, prior_sweep=spec)
    with pytest.raises(NotImplementedError, match='eval_batch'):
        single_gpu_test(model, None, pre_eval=True, device_eval=True, eval_batch=2, prior_sweep=spec)
    for own in (dict(strata=StrataSpec()), dict(errors=ErrorMaps(None)), dict(ground_dir='g'), dict(scene_dir='s')):
        with pytest.raises(NotImplementedError, match='prior_sweep with strata / errors / ground_dir / scene_dir'):
            single_gpu_test(model, None, pre_eval=True, device_eval=True, prior_sweep=spec, **own)
    with pytest.raises(TypeError, match='PriorSweep'):
        single_gpu_test(model, None, pre_eval=True, device_eval=True, prior_sweep=[(0.0, 1.0, 0)])
    ddad = types.SimpleNamespace(dataset=types.SimpleNamespace(device_protocol='ddad'))
    with pytest.raises(NotImplementedError, match='KITTI protocol'):
        single_gpu_test(model, ddad, pre_eval=True, device_eval=True, prior_sweep=spec)
    with pytest.raises(NotImplementedError, match='one device'):
        multi_gpu_test(model, None, pre_eval=True, device_eval=True, prior_sweep=spec)


def test_inference_prior_sweep_argument_errors_before_device_work():
    """A CPU model: any device work would raise something else (``torch.cuda.Stream``), so each error below comes before it."""
    from gedepth_amd.depth.apis import inference_prior_sweep
    from gedepth_amd.depth.core import PriorSweep
    frame, pe = np.zeros((375, 1242, 3), np.uint8), np.zeros((375, 1242), np.float32)
    with pytest.raises(NotImplementedError, match='DDAD'):
        inference_prior_sweep(_cpu_model('depthformer_v_ddad.py'), frame, PriorSweep(), pe=pe)
    model = _cpu_model('depthformer_swint_v.py')
    with pytest.raises(TypeError, match='PriorSweep'):
        inference_prior_sweep(model, frame, [(0.0, 1.0, 0)], pe=pe)
    with pytest.raises(TypeError, match='one frame'):
        inference_prior_sweep(model, [frame, frame], PriorSweep(), pe=pe)
    with pytest.raises(ValueError, match='no ground depth'):
        inference_prior_sweep(model, frame, PriorSweep())
    with pytest.raises(ValueError, match='smaller than the KB crop'):
        inference_prior_sweep(model, np.zeros((300, 1242, 3), np.uint8), PriorSweep(), pe=np.zeros((300, 1242), np.float32))


def test_cli_prior_sweep_arguments():
    spec = importlib.util.spec_from_file_location('tools_test_cli_sweep', os.path.join(ROOT, 'tools', 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = os.path.join(CFG, 'depthformer_swint_v.py')
    base = [cfg, '--eval', 'x', '--synthetic', '0']
    with pytest.raises(ValueError, match='--prior-sweep needs --eval and --device-eval'):
        cli.parse_args(base + ['--prior-sweep'])
    with pytest.raises(ValueError, match='need --prior-sweep'):
        cli.parse_args(base + ['--device-eval', '--sweep-pitch', '0.5'])
    for own in (['--eval-batch', '2'], ['--strata'], ['--error-dir', 'e'], ['--ground-dir', 'g'], ['--launcher', 'pytorch']):
        with pytest.raises(ValueError, match='--prior-sweep cannot be combined'):
            cli.parse_args(base + ['--device-eval', '--prior-sweep'] + own)
    with pytest.raises(ValueError, match='npz'):
        cli.parse_args(base + ['--device-eval', '--prior-sweep', '--sweep-out', 'rows.txt'])
    with pytest.raises(ValueError, match='PriorSweep'):
        cli.parse_args(base + ['--device-eval', '--prior-sweep', '--sweep-pitch', '12'])
    args = cli.parse_args(base + ['--device-eval', '--prior-sweep', '--sweep-pitch', '-0.5', '0.5', '--sweep-height', '1.05', '--sweep-no-drop',
                                  '--sweep-out', 'rows.npz'])
    sweep = cli.prior_sweep(args)
    assert sweep.names == ['baseline', 'pitch -0.50 deg', 'pitch +0.50 deg', 'height x1.05']
    assert cli.prior_sweep(cli.parse_args(base + ['--device-eval', '--prior-sweep'])).count == 6
    assert cli.prior_sweep(cli.parse_args(base)) is None
