"""The optimizer's kernels — ``ge_sumsq``, ``ge_adamw_step``, ``ge_adamw_step_shadow`` (gedepth_amd/csrc/ground.hip) — and ``FusedAdamW``
(gedepth_amd/mmrt/optim.py) at arena scale and at their edges, against float64 references computed on the GPU with plain torch operations
(tests/adamw_ref.py, which tests/test_adamw_ref_cpu.py holds against torch itself).

Sizes straddle every place the launch geometry changes: one element, the 256-thread block, the float4 body and the ``n & 3`` tail of
``sumsq_k``, the block caps (2048 blocks x 4096 elements for ``sumsq_k``, 8192 blocks x 1024 for ``adamw_k``: the grid-stride loops take a second
trip only above them), the Swin-T arena (53.5 M) and, for the reduction, the Swin-L one.

ACCURACY CRITERION of the AdamW tests.  fp32 ``torch.optim.AdamW`` (``foreach=False``) after ``clip_grad_norm_`` runs on the same inputs; both
candidates are measured against float64, per tensor (p, m, v), as ``|x - ref|_2 / |ref - before|_2`` and as the largest absolute error, and
the kernel may have at most ``FACTOR`` = 2 times torch-fp32's error (a different, equally valid fp32 operation order).  A ratio of two rounding
errors needs a population: one element's error is anywhere between 0 and an ulp for either candidate, so below 4096 elements (``POPULATION``) a
case is ``ceil(4096 / n)`` independent launches of n elements each (one common clip norm, as if they were the slices of one arena) and the errors are taken
over all of them.  The launches sit back to back in one buffer, so for odd n most of them start at an address that is not 16-byte aligned.
Parameters have std 0.02 like real weights: with O(1) parameters the rounding of the stored parameter hides the arithmetic.
Every ratio is printed (run with ``-s``).
"""
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
SUMSQ_CAP = 2048 * 4096                   # elements one sweep of sumsq_k's capped grid covers
ADAMW_CAP = 8192 * 1024                   # the same for adamw_k
SWIN_T = 53_500_000
# depthformer_a.py (Swin-L, adaptive): 444 trainable tensors, sum of numel rounded up to 64 each = 277 135 808 (277 134 755 unpadded);
# depthformer_v.py: 275 433 344.  Built on the CPU from the config, summed as GradArena does.
SWIN_L_ARENA = 277_135_808
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


# ======================================================================================================================== ge_sumsq
def _sumsq(x, out, n=None):
    from gedepth_amd import hip
    hip.call('ge_sumsq', hip.ptr(x), x.numel() if n is None else n, hip.ptr(out), hip.stream())


SUMSQ_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 4095, 4096, 4097, SUMSQ_CAP, SUMSQ_CAP + 1, SUMSQ_CAP + 2, SUMSQ_CAP + 3,
               SWIN_T + 3, SWIN_L_ARENA + 3]


@pytest.mark.parametrize('n', SUMSQ_SIZES)
def test_sumsq_vs_float64(dev, n):
    """Tolerance, derived: every term x*x is formed exactly in double (a 24-bit significand squared has 48 bits) and is non-negative, so any
    summation order has a relative error of at most (n - 1) * 2^-53; the float64 torch sum it is compared with has the same bound: 2 * n * 2^-53."""
    out = torch.zeros(1, device=dev, dtype=torch.float64)
    x = torch.empty(n, device=dev)
    tol = 2 * n * U
    for name in ('randn', '1e-25', '1e18'):
        x.normal_(generator=_gen(dev, n % 1000 + len(name)))
        if name != 'randn':
            x.abs_().add_(0.5).mul_(float(name))               # magnitudes 0.5 .. ~5 times 1e-25 / 1e18: squares far outside fp32's range
        ref = x.double().pow(2).sum().item()
        out.zero_()
        _sumsq(x, out)
        got = out.item()
        print(f'[sumsq n={n} {name}] got {got:.17e} ref {ref:.17e} rel {abs(got - ref) / ref:.2e} (bound {tol:.2e})')
        assert math.isfinite(got) and got > 0 and abs(got - ref) <= tol * ref, (name, got, ref)
    x.fill_(1.0)                                               # every partial sum is an integer below 2^53: exact in any order
    out.zero_()
    _sumsq(x, out)
    assert out.item() == float(n), ('ones', out.item(), n)
    x.zero_()                                                  # one large value in the LAST element (the tail, when n & 3): a dropped tail gives 0
    x[n - 1] = 1e6
    out.zero_()
    _sumsq(x, out)
    assert out.item() == 1e12, ('last element only', out.item())
    for k in range(1, min(n & 3, n) + 1):                      # ... and each tail position on its own
        x.zero_()
        x[n - k] = 3.0
        out.zero_()
        _sumsq(x, out)
        assert out.item() == 9.0, ('tail position', k, out.item())


def test_sumsq_accumulates_and_ignores_empty_input(dev):
    x = torch.randn(4099, device=dev, generator=_gen(dev, 5))
    out = torch.zeros(1, device=dev, dtype=torch.float64)
    _sumsq(x, out)
    once = out.item()
    _sumsq(x, out)                                             # no zeroing in between: out += sum
    assert abs(out.item() - 2 * once) <= 4 * U * 2 * once and once > 0
    out.fill_(7.25)
    _sumsq(x, out, n=0)
    assert out.item() == 7.25


def test_sumsq_refuses_a_misaligned_input_before_any_launch(dev):
    from gedepth_amd import hip
    buf = torch.ones(64, device=dev)
    out = torch.full((1,), 7.25, device=dev, dtype=torch.float64)
    for off in (1, 2, 3):
        x = buf[off:off + 8]
        assert x.data_ptr() % 16 != 0
        code = hip.lib().ge_sumsq(x.data_ptr(), 8, out.data_ptr(), hip.stream())
        assert code == BAD_ARG, code
        with pytest.raises(RuntimeError, match='bad argument'):
            hip.call('ge_sumsq', x.data_ptr(), 8, out.data_ptr(), hip.stream())
    assert hip.lib().ge_sumsq(buf.data_ptr(), -1, out.data_ptr(), hip.stream()) == BAD_ARG
    assert hip.lib().ge_sumsq(None, 8, out.data_ptr(), hip.stream()) == BAD_ARG
    assert hip.lib().ge_sumsq(buf.data_ptr(), 8, None, hip.stream()) == BAD_ARG
    torch.cuda.synchronize()
    assert out.item() == 7.25
    _sumsq(buf[4:12], out)                                     # 16-byte aligned again: accepted
    assert out.item() == 15.25


# ============================================================================================================ ge_adamw_step[_shadow]
def _hyper(dev, lr, t, max_norm):
    """The ten scalars as FusedAdamW.prepare builds them (doubles on the host, rounded to fp32 once)."""
    return torch.tensor([lr, B1, B2, EPS, WD, 1 - B1 ** t, 1 - B2 ** t, max_norm, 1 - B1, 1 - B2], dtype=torch.float32).to(dev)


def _segments(n, seed):
    """Cuts of [0, n) at random, mostly odd positions with alternating weight decay: [(begin, end, decayed)]."""
    g = torch.Generator().manual_seed(seed)
    cuts = sorted({int(c) | 1 for c in torch.randint(1, max(n, 2), (7,), generator=g).tolist() if (int(c) | 1) < n})
    edges = [0] + cuts + [n]
    first = seed % 2
    return [(a, b, (i + first) % 2 == 0) for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]


def _state(dev, total, t, seed, grads):
    """A mid-training state: std-0.02 parameters, moments of the size they have after t steps (bias-correction factors), non-zero."""
    g = _gen(dev, seed)
    p = torch.randn(total, device=dev, generator=g) * 0.02
    grad = torch.randn(total, device=dev, generator=g)
    m = torch.randn(total, device=dev, generator=g) * (0.3 * (1 - B1 ** t))
    v = (torch.rand(total, device=dev, generator=g) * 1.5 + 0.05) * (1 - B2 ** t)
    if grads == 'loguniform':
        # magnitudes 1e-30 .. 1e4 per element: g*g underflows / goes subnormal at the low end (v == 0 there: denom = eps); exact zeros in g;
        # elements that have never seen a gradient (m = v = g = 0) and elements with a tiny first gradient (m = v = 0)
        s = torch.pow(10.0, torch.rand(total, device=dev, generator=g, dtype=torch.float64) * 34 - 30).float()
        grad, m, v = grad * s, m * s, v * s * s
        kind = torch.randint(0, 8, (total,), device=dev, generator=g)
        grad[kind == 0] = 0
        for k in (1, 2):
            m[kind == k] = 0
            v[kind == k] = 0
        grad[kind == 1] = 0
    return p, grad, m, v


def _torch_fp32(p, grad, m, v, chunks, lr, t, max_norm):
    """fp32 torch.optim.AdamW + clip_grad_norm_ on the same inputs: one parameter per weight-decay segment of every launch (views of clones of
    the flat buffers, which the optimizer updates in place), the moments and the step counter planted in its state."""
    P, G, M, V = p.clone(), grad.clone(), m.clone(), v.clone()
    groups = {True: [], False: []}
    for base, segs in chunks:
        for a, b, d in segs:
            q = P[base + a:base + b].requires_grad_(True)
            q.grad = G[base + a:base + b]
            groups[d].append((q, M[base + a:base + b], V[base + a:base + b]))
    opt = torch.optim.AdamW([dict(params=[q for q, _, _ in groups[d]], weight_decay=WD if d else 0.0) for d in (True, False) if groups[d]],
                            lr=lr, betas=(B1, B2), eps=EPS, foreach=False)
    for d in groups:
        for q, mm, vv in groups[d]:
            opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=mm, exp_avg_sq=vv)
    params = [q for d in groups for q, _, _ in groups[d]]
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    opt.step()
    assert all(int(opt.state[q]['step']) == t for q in params)
    return P.detach(), M, V


def _errors(x, ref, before):
    d = x.double() - ref
    return (d.norm() / (ref - before.double()).norm()).item(), d.abs().max().item()


def _judge(tag, ours, theirs, ref, before):
    """The criterion of the module docstring for (p, m, v); returns the failures instead of asserting, so that a case prints all its ratios."""
    bad = []
    for name, x, y, r, b in zip('pmv', ours, theirs, ref, before):
        assert bool(torch.isfinite(x).all()), (tag, name, 'non-finite result')
        (kl2, kmax), (tl2, tmax) = _errors(x, r, b), _errors(y, r, b)
        print(f'[adamw {tag}] {name}: l2 kernel {kl2:.3e} torch {tl2:.3e} ratio {kl2 / max(tl2, 1e-300):.3f} | '
              f'max-abs kernel {kmax:.3e} torch {tmax:.3e} ratio {kmax / max(tmax, 1e-300):.3f}')
        if not (kl2 <= FACTOR * tl2 and kmax <= FACTOR * tmax):
            bad.append(f'{tag} {name}: l2 {kl2:.3e} vs torch-fp32 {tl2:.3e}, max-abs {kmax:.3e} vs {tmax:.3e}')
    return bad


def _launch(entry, bufs, mask, hyper, gnorm, base, n, shadow=None):
    """One direct launch on elements [base, base + n) of the flat buffers (raw addresses: most launches of an odd n start unaligned)."""
    from gedepth_amd import hip
    args = [b.data_ptr() + 4 * base for b in bufs]
    args += [mask.data_ptr() + base, hyper.data_ptr(), None if gnorm is None else gnorm.data_ptr(), n]
    if shadow is not None:
        args.append(shadow.data_ptr() + 2 * base)
    code = getattr(hip.lib(), entry)(*args, hip.stream())
    assert code == 0, (entry, code)


def _direct_case(dev, n, t, clip, grads='normal', seed=0, guard=None):
    """``clip``: the gradient norm as a multiple of max_norm (0.5 and 0.999: inactive, 1.001 and 100: active), or None for max_norm = 0."""
    K = min(max(1, -(-POPULATION[grads] // n)), 4096)
    total = K * n
    chunks = [(i * n, _segments(n, seed * 7919 + i)) for i in range(K)]
    p, grad, m, v = _state(dev, total, t, 1000 * seed + t % 997 + n % 991, grads)
    mask = torch.zeros(total, device=dev, dtype=torch.uint8)
    for base, segs in chunks:
        for a, b, d in segs:
            if d:
                mask[base + a:base + b] = 1
    norm = grad.double().pow(2).sum().sqrt().item()
    max_norm = 0.0 if clip is None else norm / clip
    gnorm = torch.full((1,), norm * norm, device=dev, dtype=torch.float64)
    hyper = _hyper(dev, LR, t, max_norm)
    before = (p, m, v)
    ref = adamw_step(p, grad, m, v, mask, LR, B1, B2, EPS, WD, t, max_norm, grad_norm=norm)[:3]
    theirs = _torch_fp32(p, grad, m, v, chunks, LR, t, max_norm)
    frame = (lambda x: guard.framed(x)) if guard is not None else (lambda x: x.clone())
    a = [frame(p), frame(grad), frame(m), frame(v)]            # shadow entry
    b = [frame(p), frame(grad), frame(m), frame(v)]            # plain entry
    mask_k, hyper_k, gnorm_k = (frame(mask), frame(hyper), frame(gnorm)) if guard is not None else (mask, hyper, gnorm)
    shadow = frame(torch.full((total,), -1.0, device=dev, dtype=torch.bfloat16))
    for base, _ in chunks:
        _launch('ge_adamw_step_shadow', a, mask_k, hyper_k, gnorm_k, base, n, shadow)
        _launch('ge_adamw_step', b, mask_k, hyper_k, gnorm_k, base, n)
    torch.cuda.synchronize()
    if guard is not None:
        guard.check()
    tag = f'n={n} x{K} t={t} clip={clip} {grads}'
    assert torch.equal(a[1], grad) and torch.equal(b[1], grad), (tag, 'the gradient was written')
    assert torch.equal(_bits(shadow), _bits(a[0].to(torch.bfloat16))), (tag, 'shadow != bf16(p)')
    for name, x, y in zip('pmv', (a[0], a[2], a[3]), (b[0], b[2], b[3])):
        assert torch.equal(_bits(x), _bits(y)), (tag, name, 'the shadow and the plain entry differ')
    assert bool((a[3] >= 0).all()), (tag, 'negative second moment')
    applied = clip_coef(norm, max_norm).item()
    assert (applied < 1) == (clip is not None and clip > 1), (tag, applied)
    return _judge(tag, (a[0], a[2], a[3]), theirs, ref, before)


# Elements a case pools before its error ratios are taken (module docstring).  With magnitudes spread over 34 decades both error measures are
# carried by the top decade, 1 element in 34, so those cases pool 32 times as many for the same effective population.  (Measured with 4096:
# n = 256, t = 2 gave m ratios of 2.65 in l2 and 3.27 in max-abs where every other size gave 0.8 - 1.25 and the 8 M - 53.5 M cases 1.02 - 1.05: the
# few largest elements decided, not the arithmetic.)  At most 4096 launches per case, which bounds n = 1 at 4096 elements.
POPULATION = {'normal': 4096, 'loguniform': 32 * 4096}
T_VALUES = (1, 2, 10, 1000, 100000)
CLIPS = (0.5, 0.999, 1.001, 100, None)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1023, 1025])
def test_adamw_step_small_sizes_vs_float64(dev, n):
    bad = []
    for t in T_VALUES:
        bad += _direct_case(dev, n, t, 100, seed=t % 7)
    for clip in CLIPS:
        bad += _direct_case(dev, n, 10, clip, seed=3)
    bad += _direct_case(dev, n, 2, 3.0, grads='loguniform', seed=4)
    bad += _direct_case(dev, n, 1000, None, grads='loguniform', seed=5)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('n', [ADAMW_CAP, ADAMW_CAP + 1, ADAMW_CAP + 777, SWIN_T])
def test_adamw_step_above_the_block_cap_vs_float64(dev, n):
    """8192 blocks x 256 threads x 4 elements = 8 388 608: at and above it the grid-stride loop runs a second trip for some (or, at 53.5 M, seven
    trips for all) threads."""
    bad = _direct_case(dev, n, 1000, 100, seed=1)
    bad += _direct_case(dev, n, 1, 0.5, seed=2)
    bad += _direct_case(dev, n, 100000, None, seed=3)
    bad += _direct_case(dev, n, 10, 1.001, seed=4)
    bad += _direct_case(dev, n, 2, 0.999, seed=5)
    bad += _direct_case(dev, n, 10, 3.0, grads='loguniform', seed=6)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('n', [1, 257, 1025, ADAMW_CAP + 777])
@pytest.mark.parametrize('poison', memguard.POISONS)
def test_adamw_and_sumsq_stay_inside_their_buffers(dev, n, poison):
    """Odd sizes with every buffer in a poisoned frame (tests/memguard.py): no guard byte changes, and — the inputs being framed too — a read
    past an input would put NaN / 3e38 into a result, which the value comparisons inside reject."""
    guard = memguard.Guard(poison)
    bad = _direct_case(dev, n, 10, 100, seed=8, guard=guard)
    assert not bad, '\n'.join(bad)
    x = guard.framed(torch.randn(n, device=dev, generator=_gen(dev, n)))
    out = guard.framed(torch.zeros(1, device=dev, dtype=torch.float64))
    _sumsq(x, out)
    guard.check()
    ref = x.double().pow(2).sum().item()
    assert abs(out.item() - ref) <= 2 * n * U * ref


def test_adamw_null_gnorm_and_zero_max_norm_mean_no_clipping(dev):
    """include/gedepth_hip.h: no clipping when max_norm <= 0 or gnorm_sq is NULL, for both entry points.  With max_norm = 0 the norm is still
    passed and must be harmless whatever it holds; with NULL a positive max_norm must not be applied."""
    n = 1025
    p, grad, m, v = _state(dev, n, 10, 77, 'normal')
    mask = (torch.arange(n, device=dev) % 3 == 0).to(torch.uint8)
    results = []
    for max_norm, gn in ((0.0, 1e12), (0.0, float('nan')), (0.0, 0.0), (0.5, None), (0.0, None), (-1.0, 1e12)):
        gnorm = None if gn is None else torch.full((1,), gn, device=dev, dtype=torch.float64)
        for entry in ('ge_adamw_step', 'ge_adamw_step_shadow'):
            bufs = [p.clone(), grad, m.clone(), v.clone()]
            shadow = torch.zeros(n, device=dev, dtype=torch.bfloat16) if entry.endswith('shadow') else None
            _launch(entry, bufs, mask, _hyper(dev, LR, 10, max_norm), gnorm, 0, n, shadow)
            results.append((bufs[0], bufs[2], bufs[3]))
    for r in results[1:]:
        for x, y in zip(results[0], r):
            assert torch.equal(_bits(x), _bits(y))
    ref = adamw_step(p, grad, m, v, mask, LR, B1, B2, EPS, WD, 10, 0.0)[:3]
    for x, r in zip(results[0], ref):
        assert float((x.double() - r).abs().max()) <= 1e-6 * float(r.abs().max())      # a sanity check; the accuracy tests are above


def test_adamw_entries_refuse_null_buffers(dev):
    from gedepth_amd import hip
    n = 8
    t = [torch.zeros(n, device=dev) for _ in range(4)]
    mask, hyper = torch.zeros(n, device=dev, dtype=torch.uint8), _hyper(dev, LR, 1, 0.0)
    shadow = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    good = [x.data_ptr() for x in t] + [mask.data_ptr(), hyper.data_ptr(), None, n]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert hip.lib().ge_adamw_step(*args, hip.stream()) == BAD_ARG
        assert hip.lib().ge_adamw_step_shadow(*args, shadow.data_ptr(), hip.stream()) == BAD_ARG
    assert hip.lib().ge_adamw_step_shadow(*good, None, hip.stream()) == BAD_ARG        # the shadow entry needs its shadow
    assert hip.lib().ge_adamw_step(*good[:7], -1, hip.stream()) == BAD_ARG
    assert hip.lib().ge_adamw_step(*good[:7], 0, hip.stream()) == 0                     # n == 0: nothing to do


# ========================================================================================================================= FusedAdamW
SHAPES = [(96, 3, 4, 4), (96,), (96,), (169, 3), (288, 96), (288,), (96, 96), (96,), (96,), (96,), (384, 96), (384,), (96, 384), (96,),
          (64, 32, 3, 3), (64,), (32, 64, 1, 1), (32,), (1, 49, 96), (192, 384), (192,), (192,), (169, 6), (576, 192), (576,), (17, 5, 3, 3),
          (1,), (7,), (63,), (65,), (128, 1, 3, 3), (255,), (256, 2), (33, 7), (129,), (5, 3, 3, 3), (1000,), (31, 31), (2, 3, 5, 7), (640,)]
CHANNELS_LAST = (14, 25)                  # indices into SHAPES: 4-D weights kept in NHWC order (GradArena._view's permuted slice view)


def _make_params(dev, seed=0, shapes=SHAPES, dtype=torch.float32):
    g = _gen(dev, seed)
    out = []
    for i, s in enumerate(shapes):
        x = (torch.randn(s, device=dev, generator=g) * 0.02).to(dtype)
        if shapes is SHAPES and i in CHANNELS_LAST:
            x = x.contiguous(memory_format=torch.channels_last)
        out.append(x.requires_grad_(True))
    return out


def _groups(params):
    """Two groups as paramwise_cfg produces them: 1-D tensors (norms, biases) and the position tables undecayed."""
    decayed = [p.dim() > 1 and p.shape[-1] not in (3, 6) for p in params]
    return [dict(params=[p for p, d in zip(params, decayed) if d], weight_decay=WD),
            dict(params=[p for p, d in zip(params, decayed) if not d], weight_decay=0.0)], decayed


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])       # logical (NCHW) element order, whatever the storage order


def _moments(opt, params):
    """exp_avg / exp_avg_sq per parameter out of a torch-layout state dict (ids run over the groups in order)."""
    sd = opt.state_dict()
    ordered = [p for g in opt.param_groups for p in g['params']]
    index = {id(p): i for i, p in enumerate(ordered)}
    return (_flat([sd['state'][index[id(p)]]['exp_avg'] for p in params]), _flat([sd['state'][index[id(p)]]['exp_avg_sq'] for p in params]))


def test_fused_adamw_scheduled_run_without_host_sync(dev):
    """300 steps, warm-up + cosine lr (a new value every step), two decay groups, 40 parameters (two channels-last), about a third of the steps
    clipped, gradients pre-generated on the device and NO host synchronisation between the steps: the 8-deep pinned ring of step scalars is
    cycled 37 times while the device is behind.  A step that picked up another step's scalars applies a wrong lr and misses the criterion."""
    from gedepth_amd.mmrt.optim import CosineAnnealingLr, FusedAdamW
    steps = 300
    ours_p, torch_p = _make_params(dev), _make_params(dev)
    groups, decayed = _groups(ours_p)
    sizes = [p.numel() for p in ours_p]
    total = sum(sizes)
    cpu = torch.Generator().manual_seed(1)
    scale = torch.exp(torch.rand(steps, generator=cpu) * 2 - 1)                  # |g| = scale * sqrt(total), scale in (1/e, e) ...
    max_norm = math.sqrt(total) * math.exp(1 / 3)                                # ... clipped where scale > e^(1/3): a third of the steps
    G = torch.randn(steps, total, device=dev, generator=_gen(dev, 2)) * scale.to(dev)[:, None]
    per_step = [[g.view(p.shape) for g, p in zip(G[i].split(sizes), ours_p)] for i in range(steps)]
    sched = CosineAnnealingLr(1e-4, steps, min_lr_ratio=1e-8, warmup='linear', warmup_iters=30, warmup_ratio=1e-3)
    p0 = _flat(ours_p).clone()
    ours = FusedAdamW(groups, lr=1e-4, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=max_norm)
    assert ours.arena.adopt and not ours_p[CHANNELS_LAST[0]].is_contiguous()
    torch.cuda.synchronize()
    for it in range(steps):                                                      # nothing in this loop waits for the device
        sched.apply(ours, it)
        ours.zero_grad()
        for p, g in zip(ours_p, per_step[it]):
            p.grad = g
        ours.step()
    last_norm = ours.last_grad_norm
    torch.cuda.synchronize()
    # fp32 torch
    ref_opt = torch.optim.AdamW(_groups(torch_p)[0], lr=1e-4, betas=(B1, B2), eps=EPS, foreach=False)
    for it in range(steps):
        sched.apply(ref_opt, it)
        for p, g in zip(torch_p, per_step[it]):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(torch_p, max_norm, foreach=False)
        ref_opt.step()
    # float64
    decay = torch.cat([torch.full((n,), d) for n, d in zip(sizes, decayed)]).to(dev)
    p, m, v = p0.double(), torch.zeros(total, device=dev, dtype=torch.float64), torch.zeros(total, device=dev, dtype=torch.float64)
    clipped, lrs = 0, set()
    for it in range(steps):
        lr = sched.lr_at(it)
        lrs.add(lr)
        p, m, v, gn = adamw_step(p, G[it], m, v, decay, lr, B1, B2, EPS, WD, it + 1, max_norm)
        clipped += int(clip_coef(gn, max_norm) < 1)
    print(f'[scheduled run] {clipped} of {steps} steps clipped, {len(lrs)} distinct lr, arena {ours.arena.numel}')
    assert 75 <= clipped <= 125 and len(lrs) == steps
    assert ours.step_count == steps
    zero = torch.zeros(total, device=dev)
    bad = _judge('scheduled 300 steps', (_flat(ours_p),) + _moments(ours, ours_p), (_flat(torch_p),) + _moments(ref_opt, torch_p),
                 (p, m, v), (p0, zero, zero))
    assert not bad, '\n'.join(bad)
    n = ours.arena.numel
    assert abs(last_norm.item() - gn.item()) <= (n + 1) * U * gn.item()
    shadow = _flat([q._ge_lp for q in ours_p])
    assert torch.equal(_bits(shadow), _bits(_flat(ours_p).to(torch.bfloat16)))


@pytest.mark.parametrize('max_grad_norm', [0.0, 1e9, 0.25])
def test_last_grad_norm_is_the_unclipped_float64_norm(dev, max_grad_norm):
    """ge_sumsq's bound (2 n 2^-53 relative on the sum of squares, the reference's share included) through the square root: half of it, plus
    one rounding of the root."""
    from gedepth_amd.mmrt.optim import FusedAdamW
    params = _make_params(dev, seed=4)
    opt = FusedAdamW(_groups(params)[0], lr=1e-4, max_grad_norm=max_grad_norm)
    for step in range(2):
        opt.zero_grad()
        grads = [torch.randn(p.shape, device=dev, generator=_gen(dev, 10 + step)) * (3.0 + step) for p in params]
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
        ref = _flat(grads).double().pow(2).sum().sqrt().item()
        got = opt.last_grad_norm
        assert got.dtype == torch.float64 and got.is_cuda
        assert abs(got.item() - ref) <= (opt.arena.numel + 1) * U * ref, (step, got.item(), ref)
        assert max_grad_norm in (0.0, 1e9) or ref > max_grad_norm                 # 0.25: the step was clipped


def test_fused_adamw_one_step_on_a_swin_t_sized_parameter(dev):
    """One 53.5 M-element parameter through the public API (GradArena, collect, the shadow), first step from zero moments, clipping active."""
    from gedepth_amd.mmrt.optim import FusedAdamW
    g = _gen(dev, 21)
    p = (torch.randn(SWIN_T, device=dev, generator=g) * 0.02).requires_grad_(True)
    q = p.detach().clone().requires_grad_(True)
    p0 = p.detach().clone()
    grad = torch.randn(SWIN_T, device=dev, generator=g)
    norm = grad.double().pow(2).sum().sqrt().item()
    max_norm = norm / 3
    opt = FusedAdamW([dict(params=[p], weight_decay=WD)], lr=LR, betas=(B1, B2), eps=EPS, max_grad_norm=max_norm)
    assert opt.arena.numel == SWIN_T + 32 and opt.arena.numel % 64 == 0
    opt.zero_grad()
    p.grad = grad
    opt.step()
    ref_opt = torch.optim.AdamW([dict(params=[q], weight_decay=WD)], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    q.grad = grad.clone()
    torch.nn.utils.clip_grad_norm_([q], max_norm, foreach=False)
    ref_opt.step()
    zero = torch.zeros(SWIN_T, device=dev)
    ref = adamw_step(p0, grad, zero, zero, torch.ones(SWIN_T, device=dev, dtype=torch.bool), LR, B1, B2, EPS, WD, 1, max_norm)
    assert abs(opt.last_grad_norm.item() - norm) <= (opt.arena.numel + 1) * U * norm
    bad = _judge('FusedAdamW 53.5 M', (p.detach(),) + _moments(opt, [p]), (q.detach(),) + _moments(ref_opt, [q]), ref[:3], (p0, zero, zero))
    assert not bad, '\n'.join(bad)
    assert torch.equal(_bits(p._ge_lp), _bits(p.detach().to(torch.bfloat16)))
    tail = slice(SWIN_T, SWIN_T + 32)                                             # the alignment padding stays zero
    assert not opt.arena.flat_param[tail].any() and not opt.exp_avg[tail].any() and not opt.exp_avg_sq[tail].any()


def _one_step_pair(dev, poke, max_norm=0.5):
    """The same step on FusedAdamW and on clip_grad_norm_ + torch.optim.AdamW, with ``poke`` applied to the gradient of parameter 2."""
    from gedepth_amd.mmrt.optim import FusedAdamW
    shapes = [(33, 7), (129,), (5, 3, 3, 3), (1,)]
    ours_p, torch_p = _make_params(dev, 6, shapes), _make_params(dev, 6, shapes)
    mk = lambda ps: [dict(params=ps[:2], weight_decay=WD), dict(params=ps[2:], weight_decay=0.0)]
    ours = FusedAdamW(mk(ours_p), lr=1e-3, betas=(B1, B2), max_grad_norm=max_norm)
    ref = torch.optim.AdamW(mk(torch_p), lr=1e-3, betas=(B1, B2), foreach=False)
    grads = [torch.randn(s, device=dev, generator=_gen(dev, 30 + i)) for i, s in enumerate(shapes)]
    grads[2].view(-1)[17] = poke
    ours.zero_grad()
    for p, q, g in zip(ours_p, torch_p, grads):
        p.grad = g.clone()
        q.grad = g.clone()
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(torch_p, max_norm, foreach=False)
    ours.step()
    ref.step()
    torch.cuda.synchronize()
    return ours, _flat(ours_p), _flat(torch_p), 33 * 7 + 129 + 17


def test_fused_adamw_inf_gradient_matches_torch(dev):
    """An infinite norm makes the clip factor 0: inf * 0 = NaN for the infinite element, every other gradient becomes 0 (weight decay only)."""
    ours, a, b, at = _one_step_pair(dev, float('inf'))
    assert not torch.isfinite(ours.last_grad_norm).item()
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    assert torch.isnan(a).nonzero().flatten().tolist() == [at]
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-7, equal_nan=True)


def test_fused_adamw_nan_gradient_poisons_every_parameter_like_torch(dev):
    """DECISION (FusedAdamW docstring): a NaN gradient element makes the norm and the clip factor NaN, as torch's clamp does, so every parameter
    becomes NaN — not only the element concerned while all others take a full unclipped step, which is what fminf gave."""
    ours, a, b, at = _one_step_pair(dev, float('nan'))
    assert torch.isnan(ours.last_grad_norm).item()
    assert bool(torch.isnan(b).all()), 'torch: clamp propagates the NaN norm to every gradient'
    assert bool(torch.isnan(a).all()), f'{int(torch.isnan(a).sum())} of {a.numel()} parameters are NaN'
    # without clipping there is no norm in the arithmetic: only the element itself is lost, in both
    ours, a, b, at = _one_step_pair(dev, float('nan'), max_norm=0.0)
    assert torch.isnan(ours.last_grad_norm).item()
    assert torch.isnan(a).nonzero().flatten().tolist() == [at]


def test_fused_adamw_parameter_without_gradient_is_stepped_with_a_zero_gradient(dev):
    """DECISION (FusedAdamW docstring): a parameter whose ``.grad`` is None (adopt mode) is treated as having a zero gradient — it takes weight
    decay, where torch leaves it untouched.  Pinned here for 3 steps on a decayed parameter; every other parameter follows torch."""
    from gedepth_amd.mmrt.optim import FusedAdamW
    shapes = [(33, 7), (40, 3, 2), (129,), (5, 3, 3, 3)]
    ours_p, torch_p = _make_params(dev, 8, shapes), _make_params(dev, 8, shapes)
    mk = lambda ps: [dict(params=ps[:2], weight_decay=WD), dict(params=ps[2:], weight_decay=0.0)]
    lr = 1e-2
    ours = FusedAdamW(mk(ours_p), lr=lr, betas=(B1, B2), max_grad_norm=5.0)
    ref = torch.optim.AdamW(mk(torch_p), lr=lr, betas=(B1, B2), foreach=False)
    assert ours.arena.adopt
    start = ours_p[1].detach().clone()
    for step in range(3):
        ours.zero_grad()
        ref.zero_grad(set_to_none=True)
        for i, (p, q) in enumerate(zip(ours_p, torch_p)):
            if i == 1:
                continue
            g = torch.randn(p.shape, device=dev, generator=_gen(dev, 40 + 10 * step + i))
            p.grad, q.grad = g.clone(), g.clone()
        assert ours_p[1].grad is None and torch_p[1].grad is None
        torch.nn.utils.clip_grad_norm_(torch_p, 5.0, foreach=False)
        ours.step()
        ref.step()
    for i in (0, 2, 3):
        assert torch.allclose(ours_p[i], torch_p[i], rtol=1e-5, atol=1e-7), i
    assert torch.equal(torch_p[1], start), 'torch skips a parameter without a gradient'
    expect = start.double() * (1 - lr * WD) ** 3
    assert torch.allclose(ours_p[1].double(), expect, rtol=1e-6, atol=0)
    assert not torch.equal(ours_p[1], start)
    m, v = _moments(ours, [ours_p[1]])
    assert not m.any() and not v.any()


@pytest.mark.parametrize('cfg_name', ['depthformer_swint_v.py', 'depthformer_swint_a.py'])
def test_every_trainable_parameter_of_the_swin_t_models_receives_a_gradient(dev, cfg_name):
    """What the decision above rests on: in a training step of the real models no trainable parameter is left without a gradient, so the
    zero-gradient treatment never applies to them."""
    from gedepth_amd.depth.datasets.synthetic import synthetic_batch
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    from gedepth_amd.mmrt.optim import build_optimizer
    from oracle.fill import load_filled
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'depthformer', cfg_name))
    cfg.model.pretrained = None
    model = build_depther(cfg.model)
    load_filled(model, 'optim_no_grad')
    model = model.to(dev).train()
    opt = build_optimizer(model, cfg.optimizer, cfg.optimizer_config.get('grad_clip'))
    assert opt.arena.adopt
    batch = synthetic_batch(2, 64, 96, seed=3, device=dev, valid_fraction=0.3)
    opt.zero_grad()
    out = model.train_step(batch, opt)
    out['loss'].backward()
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    print(f'[no-gradient parameters] {cfg_name}: {len(missing)} of {len(opt.arena.params)} trainable without a gradient: {missing}; '
          f'{len(frozen)} frozen')
    opt.step()
    assert missing == []
    assert math.isfinite(opt.last_grad_norm.item())


def test_fused_adamw_refuses_unequal_learning_rates(dev):
    """paramwise_groups honours lr_mult; FusedAdamW has one lr for the arena: NotImplementedError at construction, and at the step that meets a
    later edit of param_groups (a real exception: it survives ``python -O``)."""
    from gedepth_amd.mmrt.optim import FusedAdamW, paramwise_groups
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4)).to(dev)
    groups = paramwise_groups(model, 1e-3, WD, dict(custom_keys={'1.': dict(lr_mult=0.1, decay_mult=0.0)}))
    assert len({g['lr'] for g in groups}) == 2
    with pytest.raises(NotImplementedError, match='learning rate'):
        FusedAdamW(groups, lr=1e-3, weight_decay=WD)
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4)).to(dev)
    opt = FusedAdamW(paramwise_groups(model, 1e-3, WD, dict(custom_keys={'1.': dict(decay_mult=0.0)})), lr=1e-3, weight_decay=WD)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    before = [p.detach().clone() for p in model.parameters()]
    opt.param_groups[-1]['lr'] = 5e-4
    with pytest.raises(NotImplementedError, match='learning rate'):
        opt.step()
    with pytest.raises(NotImplementedError, match='learning rate'):
        opt.prepare()
    assert opt.step_count == 1
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    for g in opt.param_groups:
        g['lr'] = 5e-4
    opt.step()
    assert opt.step_count == 2
