"""Gradient accumulation on the MI355X: ``ge_grad_accum`` (gedepth_amd/csrc/accum.hip) at the sizes where its launch geometry changes,
``FusedAdamW.accumulate`` against a plain step on the summed gradient, one accumulated step of the Swin-T model and
``GradientCumulativeOptimizerHook`` in the runner.  References are plain torch operations on the device and tests/adamw_ref.py.

The kernel's launch constants (csrc/accum.hip): 256 threads, 4 float4 per thread and trip = 4096 elements per workgroup and trip, at most
2048 workgroups: ``CAP`` = 2048 * 4096 elements is what one trip of the capped grid covers; above it the unrolled loop takes a second trip.

ACCURACY CRITERION of the optimizer tests: the one tests/test_optim_gpu.py states.  fp32 ``torch.optim.AdamW`` after ``clip_grad_norm_`` runs
on the same inputs; both candidates are measured against float64 (tests/adamw_ref.py) per tensor (p, m, v) as ``|x - ref|_2 / |ref - before|_2``
and as the largest absolute error over a population of at least 4096 elements, and the kernel may have at most ``FACTOR`` = 2 times
torch-fp32's error.  ``last_grad_norm`` is held to that file's bound, (numel + 1) 2^-53 relative.  Every ratio is printed (run with ``-s``)."""
import math
import os

import pytest
import torch

import memguard
from adamw_ref import adamw_step, clip_coef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 10001
U = 2.0 ** -53
FACTOR = 2.0
ACC_THREADS, ACC_UNROLL, ACC_MAX_BLOCKS = 256, 4, 2048        # csrc/accum.hip
CAP = ACC_MAX_BLOCKS * ACC_THREADS * ACC_UNROLL * 4           # 8 388 608 elements per trip of the capped grid
SWIN_T = 53_500_003
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 4095, 4096, 4097, CAP, CAP + 1, CAP + 2, CAP + 3, SWIN_T]
LR, B1, B2, EPS, WD = 7.3e-5, 0.9, 0.999, 1e-8, 0.01


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()                   # fail loudly if the native library is missing
    return torch.device('cuda:0')


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _accum(acc, grad, first, out=None, n=None):
    from gedepth_amd import hip
    hip.call('ge_grad_accum', hip.ptr(acc), hip.ptr(grad), grad.numel() if n is None else n, int(first), hip.ptr(out), hip.stream())


# ===================================================================================================================== ge_grad_accum
@pytest.mark.parametrize('n', SIZES)
def test_grad_accum_bits_and_norm(dev, n):
    """first = 1 onto NaN, then two adds: the bits of ((g1) + g2) + g3 in torch fp32, in that order.  The squared norm against float64 within
    2 n 2^-53 relative, the bound derived in test_optim_gpu.py::test_sumsq_vs_float64 (exact squares, non-negative terms, the reference's
    share included)."""
    g1, g2, g3 = (torch.randn(n, device=dev, generator=_gen(dev, n % 1000 + k)) for k in range(3))
    out = torch.zeros(1, device=dev, dtype=torch.float64)
    tol = 2 * n * U

    def norm_ok(tag, acc):
        ref = acc.double().pow(2).sum().item()
        got = out.item()
        print(f'[grad_accum n={n} {tag}] sumsq {got:.17e} ref {ref:.17e} rel {abs(got - ref) / ref:.2e} (bound {tol:.2e})')
        assert math.isfinite(got) and got > 0 and abs(got - ref) <= tol * ref, (tag, got, ref)
    acc = torch.full((n,), float('nan'), device=dev)
    _accum(acc, g1, 1)
    assert _same_bits(acc, g1), 'first: acc = grad, the old NaN never read'
    acc.fill_(float('nan'))
    _accum(acc, g1, 1, out)                                    # the same with the norm
    assert _same_bits(acc, g1)
    norm_ok('first', acc)
    acc0 = acc.clone()
    _accum(acc, g2, 0)
    assert _same_bits(acc, torch.add(acc0, g2)), 'acc + grad: one fp32 add per element'
    out.zero_()
    _accum(acc, g3, 0, out)
    assert _same_bits(acc, (g1 + g2) + g3), 'three calls in a row'
    norm_ok('add', acc)
    assert _same_bits(g1, torch.randn(n, device=dev, generator=_gen(dev, n % 1000))), 'the gradient was written'
    # exact: acc0 = g = 1 -> every stored value is 2, every partial sum an integer below 2^53
    acc.fill_(1.0)
    g1.fill_(1.0)
    out.zero_()
    _accum(acc, g1, 0, out)
    assert out.item() == 4.0 * n and bool((acc == 2.0).all()), ('ones', out.item(), n)
    # one non-zero value at each tail position (and at the last element whatever n & 3): a dropped tail stores or sums nothing
    for k in sorted({1} | set(range(1, min(n & 3, n) + 1))):
        for first in (1, 0):
            g1.zero_()
            g1[n - k] = 3.0
            acc.fill_(float('nan')) if first else acc.zero_()
            out.zero_()
            _accum(acc, g1, first, out)
            assert out.item() == 9.0 and acc[n - k].item() == 3.0 and int(torch.count_nonzero(acc)) == 1, ('tail position', k, first, out.item())


def test_grad_accum_null_sumsq_touches_nothing_else(dev):
    """acc | a poisoned float64 | grad in one allocation: without ``sumsq`` the scalar between the buffers keeps its bits, for both kernels."""
    n = 4100
    buf = torch.randn(2 * n + 4, device=dev, generator=_gen(dev, 3))
    acc, scalar, grad = buf[:n], buf[n:n + 2], buf[n + 4:]
    assert acc.data_ptr() % 16 == 0 and grad.data_ptr() % 16 == 0 and scalar.data_ptr() % 8 == 0
    _bits(scalar).fill_(-1)                                    # 0xFFFFFFFF twice: a float64 NaN
    g, a0 = grad.clone(), acc.clone()
    _accum(acc, grad, 0)
    assert _same_bits(acc, a0 + g)
    _accum(acc, grad, 1)
    assert _same_bits(acc, g) and _same_bits(grad, g)
    assert _bits(scalar).tolist() == [-1, -1]


def test_grad_accum_ignores_empty_input(dev):
    acc, grad = torch.full((8,), 5.0, device=dev), torch.ones(8, device=dev)
    out = torch.full((1,), 7.25, device=dev, dtype=torch.float64)
    for first in (1, 0):
        _accum(acc, grad, first, out, n=0)
    assert out.item() == 7.25 and bool((acc == 5.0).all())


@pytest.mark.parametrize('n', [1025, CAP + 3])
@pytest.mark.parametrize('poison', memguard.POISONS)
def test_grad_accum_stays_inside_its_buffers(dev, n, poison):
    """Every buffer in a poisoned frame (tests/memguard.py), 8 elements longer than the call's n: no guard byte changes, acc[n:] and the
    gradient keep their bits, and a read past an input would put NaN / 3e38 into acc or the norm."""
    guard = memguard.Guard(poison)
    a0, g0 = torch.randn(n + 8, device=dev, generator=_gen(dev, 1)), torch.randn(n + 8, device=dev, generator=_gen(dev, 2))
    acc, grad = guard.framed(a0), guard.framed(g0)
    out = guard.framed(torch.zeros(1, device=dev, dtype=torch.float64))
    _accum(acc, grad, 0, out, n=n)
    _accum(acc, grad, 0, None, n=n)
    want = (a0[:n] + g0[:n]) + g0[:n]
    assert _same_bits(acc[:n], want)
    _accum(acc, grad, 1, None, n=n)
    out2 = guard.framed(torch.zeros(1, device=dev, dtype=torch.float64))
    _accum(acc, grad, 1, out2, n=n)
    guard.check()
    assert _same_bits(acc[:n], g0[:n]) and _same_bits(acc[n:], a0[n:]), 'only acc[0:n] is written'
    assert _same_bits(grad, g0), 'the gradient was written'
    for got, ref in ((out, (a0[:n] + g0[:n]).double().pow(2).sum().item()), (out2, g0[:n].double().pow(2).sum().item())):
        assert abs(got.item() - ref) <= 2 * n * U * ref


def test_grad_accum_refusals_come_before_any_launch(dev):
    from gedepth_amd import hip
    fn = hip.lib().ge_grad_accum
    buf, gbuf = torch.full((64,), 5.0, device=dev), torch.ones(64, device=dev)
    obuf = torch.full((2,), 7.25, device=dev, dtype=torch.float64)
    a, g, o, s = buf.data_ptr(), gbuf.data_ptr(), obuf.data_ptr(), hip.stream()
    assert a % 16 == 0 and g % 16 == 0 and o % 8 == 0
    refused = [(None, g, 8, o), (a, None, 8, o), (a, g, -1, o), (a, a, 8, o), (a, g, 8, o + 4)]
    refused += [(a + 4 * k, g, 8, o) for k in (1, 2, 3)] + [(a, g + 4 * k, 8, o) for k in (1, 2, 3)]
    for first in (1, 0):
        for acc, grad, n, out in refused:
            assert fn(acc, grad, n, first, out, s) == BAD_ARG, (acc, grad, n, first, out)
            if out == o:                                        # ... and without a norm (the misaligned sumsq is the one case that is then valid)
                assert fn(acc, grad, n, first, None, s) == BAD_ARG, (acc, grad, n, first)
    with pytest.raises(RuntimeError, match='bad argument'):
        hip.call('ge_grad_accum', a + 4, g, 8, 0, o, s)
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all()) and bool((gbuf == 1.0).all()) and obuf.tolist() == [7.25, 7.25]
    assert fn(a + 16, g + 32, 8, 0, o + 8, s) == 0              # aligned again: accepted
    torch.cuda.synchronize()
    assert obuf.tolist() == [7.25, 7.25 + 8 * 36.0] and bool((buf[4:12] == 6.0).all()) and int((buf == 5.0).sum()) == 56


# ======================================================================================================================== FusedAdamW
SHAPES = [(96, 3, 4, 4), (96,), (169, 3), (288, 96), (288,), (64, 32, 3, 3), (64,), (1, 49, 96), (17, 5, 3, 3), (1,), (7,), (63,), (65,),
          (255,), (33, 7), (129,), (1000,), (31, 31)]
CHANNELS_LAST = (5,)                      # index into SHAPES: a 4-D weight kept in NHWC order (GradArena._view's permuted slice view)


def _make_params(dev, seed=0):
    g = _gen(dev, seed)
    out = []
    for i, s in enumerate(SHAPES):
        x = torch.randn(s, device=dev, generator=g) * 0.02
        if i in CHANNELS_LAST:
            x = x.contiguous(memory_format=torch.channels_last)
        out.append(x.requires_grad_(True))
    return out


def _groups(params):
    decayed = [p.dim() > 1 and p.shape[-1] != 3 for p in params]
    return [dict(params=[p for p, d in zip(params, decayed) if d], weight_decay=WD),
            dict(params=[p for p, d in zip(params, decayed) if not d], weight_decay=0.0)], decayed


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])       # logical (NCHW) element order, whatever the storage order


def _moments(opt, params):
    sd = opt.state_dict()
    index = {id(p): i for i, p in enumerate(p for g in opt.param_groups for p in g['params'])}
    return (_flat([sd['state'][index[id(p)]]['exp_avg'] for p in params]), _flat([sd['state'][index[id(p)]]['exp_avg_sq'] for p in params]))


def _grad_sets(dev, sets, seed=50, scale=1.0):
    return [[torch.randn(s, device=dev, generator=_gen(dev, seed + 100 * k + i)) * scale for i, s in enumerate(SHAPES)] for k in range(sets)]


def _sequential_sum(sets):
    total = [g.clone() for g in sets[0]]
    for gs in sets[1:]:
        total = [t + g for t, g in zip(total, gs)]               # fp32, in order: ((g1) + g2) + g3
    return total


def _fused(dev, max_grad_norm, seed=0):
    from gedepth_amd.mmrt.optim import FusedAdamW
    params = _make_params(dev, seed)
    opt = FusedAdamW(_groups(params)[0], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=max_grad_norm)
    assert opt.arena.adopt and not params[CHANNELS_LAST[0]].is_contiguous() and opt.arena.numel % 64 == 0
    return opt, params


def _window(opt, params, sets, last=True):
    """The accumulating route: each set assigned to ``p.grad`` and accumulated, ``last`` on the final one, then one step."""
    for k, gs in enumerate(sets):
        opt.zero_grad()
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.accumulate(last=last and k == len(sets) - 1)
    opt.step()


def _plain(opt, params, total):
    """The parent's route: one plain step on the summed gradient."""
    opt.zero_grad()
    for p, g in zip(params, total):
        p.grad = g.clone()
    opt.step()


def _arenas(opt):
    return dict(param=opt.arena.flat_param, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, shadow=opt.arena.flat_shadow)


def _assert_bit_equal(a, b, tag):
    for (name, x), y in zip(_arenas(a).items(), _arenas(b).values()):
        assert _same_bits(x, y), (tag, name, int((_bits(x) != _bits(y)).sum()))


@pytest.mark.parametrize('clip', ['off', 'inactive'])
def test_accumulated_step_is_bit_equal_to_a_plain_step_on_the_sum(dev, clip):
    """max_grad_norm = 0, or 10^6 times the norm (the clip factor is then exactly 1 whatever the last bits of the norm, which the two routes
    reduce in different orders): parameters, both moments and the bf16 shadow carry the same bits."""
    sets = _grad_sets(dev, 3)
    total = _sequential_sum(sets)
    norm = _flat(total).double().pow(2).sum().sqrt().item()
    max_norm = 0.0 if clip == 'off' else 1e6 * norm
    A, pa = _fused(dev, max_norm)
    B, pb = _fused(dev, max_norm)
    assert getattr(A.arena, 'flat_accum', None) is None
    _window(A, pa, sets)
    _plain(B, pb, total)
    assert getattr(B.arena, 'flat_accum', None) is None, 'the plain route allocates no second arena'
    assert A.arena.flat_accum.shape == A.arena.flat_grad.shape and A.arena.flat_accum.dtype == torch.float32
    _assert_bit_equal(A, B, clip)
    assert A.step_count == B.step_count == 1
    assert not _same_bits(_flat(pa), _flat(_make_params(dev, 0))), 'the step moved the parameters'
    n = A.arena.numel
    for opt in (A, B):
        assert abs(opt.last_grad_norm.item() - norm) <= (n + 1) * U * norm
    assert _same_bits(A.arena.flat_shadow, A.arena.flat_param.to(torch.bfloat16))


def _errors(x, ref, before):
    d = x.double() - ref
    return (d.norm() / (ref - before.double()).norm()).item(), d.abs().max().item()


def _judge(tag, ours, theirs, ref, before):
    bad = []
    for name, x, y, r, b in zip('pmv', ours, theirs, ref, before):
        assert x.numel() >= 4096 and bool(torch.isfinite(x).all()), (tag, name)
        (kl2, kmax), (tl2, tmax) = _errors(x, r, b), _errors(y, r, b)
        print(f'[accum adamw {tag}] {name}: l2 kernel {kl2:.3e} torch {tl2:.3e} ratio {kl2 / max(tl2, 1e-300):.3f} | '
              f'max-abs kernel {kmax:.3e} torch {tmax:.3e} ratio {kmax / max(tmax, 1e-300):.3f}')
        if not (kl2 <= FACTOR * tl2 and kmax <= FACTOR * tmax):
            bad.append(f'{tag} {name}: l2 {kl2:.3e} vs torch-fp32 {tl2:.3e}, max-abs {kmax:.3e} vs {tmax:.3e}')
    return bad


def _torch_steps(dev, totals, max_norm):
    """fp32 ``clip_grad_norm_`` + ``torch.optim.AdamW`` on the summed gradients, one step per entry of ``totals``."""
    params = _make_params(dev, 0)
    opt = torch.optim.AdamW(_groups(params)[0], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    for total in totals:
        for p, g in zip(params, total):
            p.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
        opt.step()
    return params, opt


def _float64_steps(dev, totals, max_norm, t0=1):
    params = _make_params(dev, 0)
    decay = torch.cat([torch.full((p.numel(),), d) for p, d in zip(params, _groups(params)[1])]).to(dev)
    p = _flat(params).double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    gn = None
    for k, total in enumerate(totals):
        p, m, v, gn = adamw_step(p, _flat(total), m, v, decay, LR, B1, B2, EPS, WD, t0 + k, max_norm)
    return (p, m, v), gn


def test_accumulated_step_with_an_active_clip_vs_float64(dev):
    """Clipped to a third of the norm.  The accumulating route with ``last=True`` (norm from the accumulation pass), the one without (the
    ``ge_sumsq`` fallback in the step) and the plain route reduce the norm in different orders; each is held to float64 on its own."""
    sets = _grad_sets(dev, 3, seed=60)
    total = _sequential_sum(sets)
    norm = _flat(total).double().pow(2).sum().sqrt().item()
    max_norm = norm / 3
    ref, gn = _float64_steps(dev, [total], max_norm)
    assert clip_coef(gn, max_norm).item() < 0.34
    tp, topt = _torch_steps(dev, [total], max_norm)
    theirs = (_flat(tp),) + _moments(topt, tp)
    p0 = _flat(_make_params(dev, 0))
    zero = torch.zeros_like(p0)
    bad, results = [], {}
    for route in ('last', 'fallback', 'plain'):
        opt, params = _fused(dev, max_norm)
        if route == 'plain':
            _plain(opt, params, total)
        else:
            _window(opt, params, sets, last=route == 'last')
        assert opt.step_count == 1 and opt._accum_count == 0
        got = opt.last_grad_norm.item()
        assert abs(got - gn.item()) <= (opt.arena.numel + 1) * U * gn.item(), (route, got, gn.item())
        results[route] = (_flat(params),) + _moments(opt, params)
        bad += _judge(route, results[route], theirs, ref, (p0, zero, zero))
        assert _same_bits(_flat([q._ge_lp for q in params]), _flat(params).to(torch.bfloat16)), (route, 'shadow != bf16(p)')
    assert not bad, '\n'.join(bad)
    for name, x, y in zip('mv', results['last'][1:], results['fallback'][1:]):
        assert torch.allclose(x, y, rtol=1e-6, atol=0), name       # the same sum, clip factors one fp32 rounding apart at most


def test_step_count_advances_once_per_window(dev):
    """A window of three, then a window of two: ``step_count`` 1, then 2, and the second step's bias corrections use t = 2 — against float64
    under the criterion, bit-equal to two plain steps on the sums, and far from a reference whose second step used t = 5 (one count per
    accumulation)."""
    sets = _grad_sets(dev, 5, seed=70)
    totals = [_sequential_sum(sets[:3]), _sequential_sum(sets[3:])]
    A, pa = _fused(dev, 0.0)
    B, pb = _fused(dev, 0.0)
    _window(A, pa, sets[:3])
    assert A.step_count == 1
    _window(A, pa, sets[3:])
    assert A.step_count == 2
    for total in totals:
        _plain(B, pb, total)
    _assert_bit_equal(A, B, 'two windows')
    ref, _ = _float64_steps(dev, totals, 0.0)
    tp, topt = _torch_steps(dev, totals, 0.0)
    p0 = _flat(_make_params(dev, 0))
    zero = torch.zeros_like(p0)
    ours = (_flat(pa),) + _moments(A, pa)
    bad = _judge('two windows', ours, (_flat(tp),) + _moments(topt, tp), ref, (p0, zero, zero))
    assert not bad, '\n'.join(bad)
    (p1, m1, v1), _ = _float64_steps(dev, totals[:1], 0.0)
    decay = torch.cat([torch.full((p.numel(),), d) for p, d in zip(pa, _groups(pa)[1])]).to(dev)
    late = adamw_step(p1, _flat(totals[1]), m1, v1, decay, LR, B1, B2, EPS, WD, 5, 0.0)[0]      # the second step with t = 5
    right = (ours[0].double() - ref[0]).norm().item()
    assert (ours[0].double() - late).norm().item() > 100 * right, 'a step counted per accumulation (t = 5) would be told apart'


def test_inf_in_an_accumulated_gradient_behaves_like_an_inf_gradient(dev):
    """FusedAdamW's docstring: an inf element makes the norm infinite and the clip factor 0 and poisons its own element only."""
    sets = _grad_sets(dev, 3, seed=80)
    sets[1][3].view(-1)[17] = float('inf')
    at = sum(math.prod(s) for s in SHAPES[:3]) + 17
    total = _sequential_sum(sets)
    A, pa = _fused(dev, 0.5)
    B, pb = _fused(dev, 0.5)
    _window(A, pa, sets)
    _plain(B, pb, total)
    torch.cuda.synchronize()
    assert not torch.isfinite(A.last_grad_norm).item()
    a, b = _flat(pa), _flat(pb)
    assert torch.isnan(a).nonzero().flatten().tolist() == [at]
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(torch.isfinite(a[~torch.isnan(a)]).all())
    _assert_bit_equal(A, B, 'inf')                                # NaN payloads included: the same kernel on the same bits


# ======================================================================================================================= whole model
def _swin_t(dev, tag):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    from gedepth_amd.mmrt.optim import build_optimizer
    from oracle.fill import load_filled
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py'))
    cfg.model.pretrained = None
    model = build_depther(cfg.model)
    load_filled(model, tag)
    model = model.to(dev).train()
    opt = build_optimizer(model, cfg.optimizer, cfg.optimizer_config.get('grad_clip'))
    assert opt.arena.adopt
    return cfg, model, opt


def _batches(dev):
    from gedepth_amd.depth.datasets.synthetic import synthetic_batch
    return [synthetic_batch(2, 64, 96, seed=s, device=dev, valid_fraction=0.3) for s in (3, 4)]


def test_swin_t_accumulated_step_is_adamw_on_the_summed_gradients(dev):
    """N = 2 on one model: the gradients are cloned out of the arena after each backward, so forward non-determinism cannot matter."""
    from gedepth_amd import hip
    _, model, opt = _swin_t(dev, 'grad_accum')
    a = opt.arena
    grads = []
    for k, batch in enumerate(_batches(dev)):
        opt.zero_grad()
        out = model.train_step(batch, opt)
        (out['loss'] / 2).backward()
        a.collect()
        grads.append(a.flat_grad.clone())
        opt.accumulate(last=k == 1)
    assert not torch.equal(grads[0], grads[1]) and bool(torch.isfinite(grads[1]).all())
    gsum = grads[0] + grads[1]
    assert _same_bits(a.flat_accum, gsum)
    before = a.flat_param.clone()
    P, M, V, S = a.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), a.flat_shadow.clone()
    opt.step()
    assert opt.step_count == 1
    hip.call('ge_adamw_step_shadow', hip.ptr(P), hip.ptr(gsum), hip.ptr(M), hip.ptr(V), hip.ptr(opt.wd_mask), hip.ptr(opt.hyper),
             hip.ptr(opt.gnorm_sq), a.numel, hip.ptr(S), hip.stream())
    for name, x, y in (('param', a.flat_param, P), ('exp_avg', opt.exp_avg, M), ('exp_avg_sq', opt.exp_avg_sq, V), ('shadow', a.flat_shadow, S)):
        assert _same_bits(x, y), name
    norm = gsum.double().pow(2).sum().sqrt().item()
    assert abs(opt.last_grad_norm.item() - norm) <= (a.numel + 1) * U * norm
    unchanged = [i for i, (off, n) in enumerate(a.slices()) if torch.equal(a.flat_param[off:off + n], before[off:off + n])]
    assert unchanged == [], f'{len(unchanged)} of {len(a.params)} trainable parameters did not move'


def test_runner_accumulates_over_two_iterations(dev):
    """max_iters = 5, N = 2: steps after iterations 1, 3 and 4 (a final window of one), the third with the learning rate of iteration 4."""
    from gedepth_amd.mmrt.runner import GradientCumulativeOptimizerHook, IterBasedRunner
    cfg, model, opt = _swin_t(dev, 'grad_accum_runner')
    logs = []
    runner = IterBasedRunner(model, opt, logger=logs.append, max_iters=5)
    runner.register_training_hooks(dict(policy='CosineAnnealing', min_lr_ratio=1e-2, warmup='linear', warmup_iters=3, warmup_ratio=0.1, by_epoch=False),
                                   dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2, grad_clip=cfg.optimizer_config.get('grad_clip')),
                                   None, None)
    assert isinstance(runner.hooks[1], GradientCumulativeOptimizerHook)
    runner.run([_batches(dev)])
    torch.cuda.synchronize()
    assert runner.iter == 5 and opt.step_count == 3 and opt._accum_count == 0
    sched = runner.hooks[0].schedule
    lrs = {sched.lr_at(i) for i in range(5)}
    assert len(lrs) == 5
    assert opt.hyper[0].item() == torch.tensor(sched.lr_at(4), dtype=torch.float32).item()
    assert math.isfinite(float(runner.outputs['log_vars']['loss']))
    assert math.isfinite(opt.last_grad_norm.item())
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert len([m for m in logs if 'BatchNorm' in m]) == 1
