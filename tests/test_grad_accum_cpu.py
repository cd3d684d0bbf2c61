"""Gradient accumulation without a GPU: the seventh header table and the exported symbol, ``GradArena.enable_accum`` under a permutation of
the arena, the schedule of ``GradientCumulativeOptimizerHook`` (factors, boundaries, a resumed run, a short final window) against a
recording stub optimizer on a float64 model, the refusals, and the ``--cumulative-iters`` option of tools/train.py."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest
import torch

from gedepth_amd import hip
from gedepth_amd.mmrt.runner import GradientCumulativeOptimizerHook, IterBasedRunner, OptimizerHook

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_CONFIG = dict(policy='CosineAnnealing', min_lr_ratio=1e-2, by_epoch=False)


# ------------------------------------------------------------------------------------------------ header table, exported symbol
def test_accum_header_is_parsed_into_its_own_table():
    assert hip.ACCUM_HEADERS == {'ACCUM_SIGNATURES': 'gedepth_accum.h'}
    header = open(os.path.join(ROOT, 'include', 'gedepth_accum.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.ACCUM_SIGNATURES) == {'ge_grad_accum'}
    c = ctypes
    assert hip.ACCUM_SIGNATURES['ge_grad_accum'] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_long, c.c_int, c.c_void_p, c.c_void_p])
    others = {**hip.HEADERS, **hip.EXTRA_HEADERS, **hip.SCENE_HEADERS, **hip.STRATA_HEADERS, **hip.NECK_HEADERS, **hip.ERROR_HEADERS}
    for table in others:
        assert 'ge_grad_accum' not in getattr(hip, table), table


def test_library_exports_ge_grad_accum():
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    if shutil.which('nm') is None:
        pytest.fail('nm (binutils) is needed to list the dynamic symbols of the library')
    out = subprocess.run(['nm', '-D', '--defined-only', hip.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()[-2:-1] == ['T']}
    assert 'ge_grad_accum' in exported
    fn = hip.lib().ge_grad_accum                                       # lib() has bound the seventh table too
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == hip.ACCUM_SIGNATURES['ge_grad_accum'][1]
    # every check comes before a launch, so the refusals are safe without a GPU (4096 / 8192: aligned addresses that are never followed)
    assert fn(None, 4096, 8, 1, None, None) == 10001 and fn(4096, None, 8, 1, None, None) == 10001
    assert fn(4096, 8192, -1, 1, None, None) == 10001 and fn(4096, 4096, 8, 1, None, None) == 10001
    assert fn(4100, 8192, 8, 0, None, None) == 10001 and fn(4096, 8200, 8, 0, None, None) == 10001
    assert fn(4096, 8192, 8, 0, 12292, None) == 10001
    assert fn(4096, 8192, 0, 0, None, None) == 0                        # n == 0: nothing to do


# ------------------------------------------------------------------------------------------------ the second arena
def test_enable_accum_follows_its_parameters_through_permute():
    from gedepth_amd.mmrt.optim import GradArena
    shapes = [(5, 3), (70,), (4, 6, 3, 3), (1,), (65, 2)]
    params = [torch.randn(s).requires_grad_(True) for s in shapes]
    params[2] = params[2].detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    arena = GradArena(params, adopt=False)
    assert getattr(arena, 'flat_accum', None) is None
    acc = arena.enable_accum()
    assert acc is arena.enable_accum(), 'allocated once'
    assert acc.dtype == torch.float32 and acc.shape == (arena.numel,) and acc.device == arena.flat_param.device
    acc.fill_(-1.0)                                                     # the alignment padding
    for i, (off, n) in enumerate(arena.slices()):
        acc[off:off + n] = float(i + 1)
        arena.flat_param[off:off + n] = float(i + 1)
    mark = {id(p): float(i + 1) for i, p in enumerate(arena.params)}
    order = [3, 0, 4, 2, 1]
    old_offsets = list(arena.offsets)
    arena.permute(order)
    assert arena.offsets != old_offsets and arena.flat_accum is not acc
    assert arena.flat_accum.shape == (arena.numel,) and arena.flat_accum.dtype == torch.float32
    for p, (off, n) in zip(arena.params, arena.slices()):
        assert bool((arena.flat_accum[off:off + n] == mark[id(p)]).all()), (off, n)
        assert bool((p.data == mark[id(p)]).all())                      # ... where the parameter itself went
    assert int((arena.flat_accum == -1.0).sum()) == arena.numel - sum(p.numel() for p in params)
    arena.permute([1, 4, 3, 0, 2])                                      # a second permutation: the callback is still registered once
    for p, (off, n) in zip(arena.params, arena.slices()):
        assert bool((arena.flat_accum[off:off + n] == mark[id(p)]).all())
    assert len(arena._permute_callbacks) == 1


# ------------------------------------------------------------------------------------------------ the hook's schedule
class StubOptimizer:
    """Records what the hook asks of the optimizer and sums ``p.grad`` in float64, like an accumulation arena."""

    def __init__(self, params):
        self.params = list(params)
        self.defaults = dict(lr=1e-3)
        self.param_groups = [dict(params=self.params, lr=1e-3)]
        self.events, self.runner = [], None
        self.sum, self.stepped = None, []

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def _grads(self):
        return [torch.zeros_like(p, dtype=torch.float64) if p.grad is None else p.grad.detach().double().clone() for p in self.params]

    def accumulate(self, last=False):
        g = self._grads()
        self.sum = g if self.sum is None else [a + b for a, b in zip(self.sum, g)]
        self.events.append(('accumulate', self.runner.iter, bool(last), [x.clone() for x in g]))

    def step(self):
        self.stepped.append(self.sum if self.sum is not None else self._grads())
        self.sum = None
        self.events.append(('step', self.runner.iter, self.runner.current_lr))


class ScalarModel(torch.nn.Module):
    """loss = w * x with x = 1: the gradient an iteration hands over is 1 / factor."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1, dtype=torch.float64))
        self.calls = 0

    def train_step(self, batch, optimizer):
        self.calls += 1
        loss = (self.w * batch['x']).sum()
        return dict(loss=loss, log_vars=dict(loss=loss.item()), num_samples=1)


def _run(model, loader, max_iters, opt_cfg, start=0, hip_graph=False, checkpoint_config=None):
    opt = StubOptimizer(model.parameters())
    logs = []
    runner = IterBasedRunner(model, opt, logger=logs.append, max_iters=max_iters, hip_graph=hip_graph)
    opt.runner = runner
    runner.register_training_hooks(LR_CONFIG, opt_cfg, checkpoint_config, None)
    runner.iter = start
    runner.run([loader])
    return runner, opt, logs


def _schedule(opt):
    acc = [e for e in opt.events if e[0] == 'accumulate']
    factors = [round(1.0 / e[3][0].item()) for e in acc]
    return factors, [e[1] for e in opt.events if e[0] == 'step'], [e[1] for e in acc if e[2]]


ONES = [dict(x=torch.ones(1, dtype=torch.float64))]
CUMULATIVE = dict(type='GradientCumulativeOptimizerHook', cumulative_iters=3, grad_clip=dict(max_norm=35, norm_type=2))


def test_hook_schedule_with_a_short_final_window():
    runner, opt, _ = _run(ScalarModel(), ONES, 7, CUMULATIVE)
    factors, steps, lasts = _schedule(opt)
    assert factors == [3, 3, 3, 3, 3, 3, 1]
    assert steps == [2, 5, 6] and lasts == steps, 'accumulate(last=True) exactly at the boundaries'
    assert [e[:2] for e in opt.events if e[1] == 2] == [('accumulate', 2), ('step', 2)], 'the step follows its accumulate'
    assert runner.iter == 7
    sched = runner.hooks[0].schedule
    assert [e[2] for e in opt.events if e[0] == 'step'] == [sched.lr_at(i) for i in steps], 'each step takes the lr of its iteration'
    assert runner.outputs['log_vars']['loss'] == 1.0, 'log_vars keep the unscaled loss'
    assert [s[0].item() for s in opt.stepped] == [pytest.approx(1.0, abs=2 ** -50)] * 3, 'every window sums to one full gradient'


def test_hook_schedule_after_a_resume():
    runner, opt, _ = _run(ScalarModel(), ONES, 9, CUMULATIVE, start=2)
    factors, steps, lasts = _schedule(opt)
    assert steps == [4, 7, 8] and lasts == steps
    assert factors == [3, 3, 3, 3, 3, 3, 1] and factors[-1] == 1
    assert isinstance(runner.hooks[1], GradientCumulativeOptimizerHook) and runner.hooks[1].start == 2


def test_hook_two_iteration_final_window():
    _, opt, _ = _run(ScalarModel(), ONES, 5, CUMULATIVE)
    factors, steps, _ = _schedule(opt)
    assert factors == [3, 3, 3, 2, 2] and steps == [2, 4]


class LinearModel(torch.nn.Module):
    """Batch-decoupled: Linear + a mean loss, float64; every term of every gradient sum is positive (no cancellation)."""
    IN = 5

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.fc = torch.nn.Linear(self.IN, 1).double()
        with torch.no_grad():
            self.fc.weight.copy_(torch.rand(1, self.IN, generator=g, dtype=torch.float64) + 0.5)
            self.fc.bias.fill_(0.3)

    def train_step(self, batch, optimizer):
        loss = ((self.fc(batch['x']).squeeze(1) - batch['t']) ** 2).mean()
        return dict(loss=loss, log_vars=dict(loss=loss.item()), num_samples=batch['x'].shape[0])


def test_accumulated_micro_batches_equal_one_large_batch():
    """N = 3 micro-batches of b = 4 samples through the hook against one batch of N b = 12.  x, w, bias > 0 and t < 0, so every residual and
    every per-sample term of every gradient element is positive and "relative" is relative to the element itself.  n_terms = 21: an element
    is a sum of N b = 12 terms (12 roundings at most, however it is split), and each term goes through at most IN + 4 = 9 more rounded
    operations (IN products and sums of the forward, the residual, the factor 2 / count, the product with x); each rounds by at most 2^-53
    relative to a positive quantity, in either of the two evaluations: 2 * 21 * 2^-53 = n_terms * 2^-52."""
    N, b, n_terms = 3, 4, 21
    assert n_terms == N * b + LinearModel.IN + 4
    g = torch.Generator().manual_seed(12)
    x = torch.rand(N * b, LinearModel.IN, generator=g, dtype=torch.float64) + 0.5
    t = -(torch.rand(N * b, generator=g, dtype=torch.float64) + 0.5)
    micro = [dict(x=x[i * b:(i + 1) * b], t=t[i * b:(i + 1) * b]) for i in range(N)]
    model = LinearModel()
    _, opt, _ = _run(model, micro, N, dict(type='GradientCumulativeOptimizerHook', cumulative_iters=N))
    assert len(opt.stepped) == 1
    model.zero_grad()
    model.train_step(dict(x=x, t=t), None)['loss'].backward()
    for got, p in zip(opt.stepped[0], model.parameters()):
        ref = p.grad.double()
        assert bool((ref > 0).all())
        rel = ((got - ref).abs() / ref).max().item()
        print(f'[micro-batches vs one batch] {tuple(p.shape)}: max relative difference {rel:.3e} (bound {n_terms * 2.0 ** -52:.3e})')
        assert rel <= n_terms * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ refusals, N = 1, notices
def test_hip_graph_with_accumulation_is_refused_before_any_work():
    model = ScalarModel()
    with pytest.raises(NotImplementedError, match=r'--hip-graph.*cumulative_iters|cumulative_iters.*--hip-graph') as e:
        _run(model, ONES, 4, CUMULATIVE, hip_graph=True)
    assert '--hip-graph' in str(e.value) and 'cumulative_iters' in str(e.value)
    assert model.calls == 0
    hook = GradientCumulativeOptimizerHook(cumulative_iters=1)          # N = 1 is OptimizerHook: the captured step is left alone
    hook.before_run(IterBasedRunner(model, StubOptimizer(model.parameters()), max_iters=1, hip_graph=True))


def test_unknown_optimizer_hook_type_raises_key_error():
    model = ScalarModel()
    runner = IterBasedRunner(model, StubOptimizer(model.parameters()), max_iters=1)
    with pytest.raises(KeyError, match='NoSuchOptimizerHook'):
        runner.register_training_hooks(LR_CONFIG, dict(type='NoSuchOptimizerHook'), None, None)
    runner.register_training_hooks(LR_CONFIG, dict(grad_clip=None), None, None)           # the default type
    assert type(runner.hooks[-1]) is OptimizerHook
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match='cumulative_iters'):
            GradientCumulativeOptimizerHook(cumulative_iters=bad)


def test_one_cumulative_iter_is_the_plain_optimizer_hook():
    plain = _run(ScalarModel(), ONES, 4, dict(grad_clip=None))[1]
    one = _run(ScalarModel(), ONES, 4, dict(type='GradientCumulativeOptimizerHook', cumulative_iters=1, grad_clip=None))[1]
    assert [e[0] for e in one.events] == ['step'] * 4, 'accumulate is never called'
    assert one.events == plain.events
    assert [s[0].item() for s in one.stepped] == [1.0] * 4 == [s[0].item() for s in plain.stepped]


def test_batchnorm_and_checkpoint_interval_are_mentioned_once():
    class WithBN(ScalarModel):
        def __init__(self):
            super().__init__()
            self.bn = torch.nn.BatchNorm1d(2)
    _, _, logs = _run(WithBN(), ONES, 3, CUMULATIVE, checkpoint_config=dict(interval=4, by_epoch=False))
    assert len([m for m in logs if 'BatchNorm' in m]) == 1 and len([m for m in logs if 'checkpoint interval 4' in m]) == 1
    _, _, logs = _run(ScalarModel(), ONES, 3, CUMULATIVE, checkpoint_config=dict(interval=6, by_epoch=False))
    assert not [m for m in logs if 'BatchNorm' in m or 'checkpoint' in m]


# ------------------------------------------------------------------------------------------------ tools/train.py
def test_train_cli_cumulative_iters_rewrites_the_optimizer_config(monkeypatch):
    from gedepth_amd.mmrt.config import Config
    monkeypatch.setenv('DEBUG_CLR_GRAPH_PACKET_CAPTURE', os.environ.get('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0'))      # the tool sets it at import
    spec = importlib.util.spec_from_file_location('tools_train_cli_accum', os.path.join(ROOT, 'tools', 'train.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parse_args(['cfg.py']).cumulative_iters == 1
    args = cli.parse_args(['cfg.py', '--cumulative-iters', '4'])
    assert args.cumulative_iters == 4
    path = os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py')
    cfg = Config.fromfile(path)
    clip = cfg.to_dict()['optimizer_config']['grad_clip']
    assert clip == dict(max_norm=35, norm_type=2)
    cli.set_cumulative_iters(cfg, args.cumulative_iters)
    assert cfg.to_dict()['optimizer_config'] == dict(type='GradientCumulativeOptimizerHook', cumulative_iters=4, grad_clip=clip)
    same = Config.fromfile(path)
    cli.set_cumulative_iters(same, 1)
    assert same.to_dict()['optimizer_config'] == Config.fromfile(path).to_dict()['optimizer_config']
    with pytest.raises(ValueError, match='cumulative-iters'):
        cli.set_cumulative_iters(same, 0)
