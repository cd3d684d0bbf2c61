"""The window-attention kernels (gedepth_amd/csrc/window_attn.hip: variant 1, exact fp32; window_attn_mfma.hip: variant 2, bf16 MFMA, what bf16
training runs; variant 3, fp8 forward) through ``gedepth_amd.kernels.window_attention``, forward and backward, against tests/winattn_ref.py:

a. routed inputs, bit for bit: every query attends to exactly one key, so out is a gather of v, d_v the inverse gather of d_out and every other
   gradient exactly 0 in every arithmetic.  Pins the window partition, the roll, the region ids, the key permutation inside an MFMA K-step, both
   LDS transposes and the pad rows.
b. the mask is an additive -100: a score of 362 in another region still wins (bit for bit); one of 23 loses (against float64).
c. stress inputs (peaked softmax, a common offset on k, an offset on v, a large bias table) against the float64 reference.
d. many windows per persistent workgroup, unevenly divided: the register-held bias-table gradient summed over 3 and 4 windows; routing there
   bit for bit (the double-buffered token tables of the two-wave backward) and bit-identical gradients over repeated runs.
e. fp8: all-zero q and v tiles.

Tolerances of b - d are not constants.  The budget of a (case, tensor) pair is the error of ``winattn_ref.model`` — the same computation on the CPU
in the kernel's arithmetic (float32, or float32 with the MFMA kernels' bf16 roundings) — against the float64 ``winattn_ref.core``, as l2rel and as
max-abs error over the tensor's maximum; the kernel's error against ``core`` (not against the model) must stay within 2x that on both measures
(the factor covers float32 summation order and the hardware exp, orders below a bf16 step).  Variant 1 on float32 storage takes the larger of
that and the suite's RTOL = 1e-4, ATOL = 1e-5.  Every test prints its kernel / budget ratios.

Worst kernel / budget ratios observed on MI355X (l2rel, max/scale) are recorded next to the case tables below.  In short: variant 2 sits at
1.00 on out, d_qkv and d_qkv_bias everywhere (its error IS the bf16 roundings the model makes) and at 0.7 - 1.9 on d_table, which no bf16 rounding
touches in the kernel or in the model, so both are at float32 level (1e-7 .. 1e-5); variant 1 on float32 is at 0.7 - 4.8 of the float32 model's
1e-7 .. 1e-5, i.e. at most 2.4e-5 absolute, under the suite's 1e-4."""
import functools

import pytest
import torch

import winattn_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5        # the suite's fp32 tolerance (test_kernels_gpu.py)
SCALE = 32 ** -0.5

# (B, H, W, nH)                   what it hits
GEOMS = [(2, 3, 5, 3),          # one window, pads on both sides; with shift, all nine regions inside it
         (1, 7, 7, 3),          # one window, no pad
         (1, 8, 15, 6),         # last window row and column hold one real row / column and six pad ones
         (2, 13, 6, 12),        # W < 7, H = 14 - 1
         (1, 14, 21, 24)]       # exact multiples: no pads, masks only

# variant, storage
RUNS = [(1, torch.float32), (1, torch.bfloat16), (2, torch.bfloat16), (3, torch.bfloat16)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()                   # fail loudly if the native library is missing
    return torch.device('cuda:0')


def gen(seed):
    return torch.Generator().manual_seed(seed)


def run_kernel(dev, qkv, qb, tab, go, H, W, nH, shift, variant, dt, backward=True):
    """-> out, d_qkv, d_qkv_bias, d_table on the CPU in float64 (gradients None without ``backward``)."""
    from gedepth_amd.kernels import window_attention
    q = qkv.to(dt).to(dev).requires_grad_(True)
    b = qb.float().to(dev).requires_grad_(True)
    t = tab.float().to(dev).requires_grad_(True)
    o = window_attention(q, b, t, H, W, nH, shift, SCALE, variant)
    if not backward:
        return o.detach().double().cpu(), None, None, None
    o.backward(go.to(dt).to(dev))
    return tuple(x.detach().double().cpu() for x in (o, q.grad, b.grad, t.grad))


def reference(qkv, qb, tab, go, H, W, nH, shift):
    """float64 ``core`` and its autograd gradients."""
    q, b, t = (x.double().clone().requires_grad_(True) for x in (qkv, qb, tab))
    o = R.core(q, b, t, H, W, nH, shift, SCALE)
    o.backward(go.double())
    return o.detach(), q.grad, b.grad, t.grad


NAMES = ('out', 'd_qkv', 'd_qkv_bias', 'd_table')


def check_budget(label, got, ref, mod, f32, n=4):
    """kernel error against float64 within 2x the model's error against float64, per tensor and on both measures; prints the ratios."""
    failures = []
    for name, a, r, m in list(zip(NAMES, got, ref, mod))[:n]:
        assert bool(torch.isfinite(a).all()), f'{label} {name}: non-finite'
        (l2, mx), (bl2, bmx) = R.errors(a, r), R.errors(m, r)
        lim_l2, lim_mx = 2 * bl2, 2 * bmx
        scale = r.abs().max().item()
        if f32 and scale > 0:
            lim_l2, lim_mx = max(lim_l2, RTOL), max(lim_mx, RTOL + ATOL / scale)
        ratio = [e / b if b > 0 else (0.0 if e == 0 else float('inf')) for e, b in ((l2, bl2), (mx, bmx))]
        print(f'[winattn {label}] {name}: l2rel {l2:.2e} (model {bl2:.2e}, ratio {ratio[0]:.2f})  max/scale {mx:.2e} (model {bmx:.2e}, ratio {ratio[1]:.2f})')
        if not (l2 <= lim_l2 and mx <= lim_mx):
            failures.append(f'{name}: l2rel {l2:.3e} > {lim_l2:.3e} or max/scale {mx:.3e} > {lim_mx:.3e}')
    assert not failures, f'{label}: ' + '; '.join(failures)


def bf16_exact(x):
    return x.bfloat16().double()


# ================================================================================ a. routing, bit for bit
@functools.lru_cache(maxsize=None)
def _routed(geom, shift, amplitude, cross):
    B, H, W, nH = geom
    r = R.routed_inputs(B, H, W, nH, shift, seed=H * 100 + W + shift, amplitude=amplitude, cross_region=cross)
    tab = (torch.rand(169, nH, generator=gen(21), dtype=torch.float64) * 2 - 1) * 2                  # magnitude 2
    return r, tab.float().double()


@pytest.mark.parametrize('geom', GEOMS)
@pytest.mark.parametrize('shift', [0, 3])
def test_routing_bit_for_bit(dev, geom, shift):
    """Expected values are exact gathers (winattn_ref.routed_inputs; the float64 reference, itself held to the oracle on the CPU, gives the same
    to 1e-100): any difference is a routing error of the kernel."""
    B, H, W, nH = geom
    C = nH * 32
    r, tab = _routed(geom, shift, 8, False)
    for variant, dt in RUNS:
        what = f'variant {variant} {dt} {geom} shift {shift}'
        o, dqkv, dqb, dtab = run_kernel(dev, r['qkv'], r['qkv_bias'], tab, r['go'], H, W, nH, shift, variant, dt)
        for x in (o, dqkv, dqb, dtab):
            assert bool(torch.isfinite(x).all()), what
        assert torch.equal(o, r['out']), f'{what}: out is not the gather, {int((o != r["out"]).sum())} elements differ'
        assert torch.equal(dqkv[:, :, 2 * C:], r['dv']), f'{what}: d_v is not the inverse gather, {int((dqkv[:, :, 2 * C:] != r["dv"]).sum())} elements differ'
        assert not bool(dqkv[:, :, :C].any()), f'{what}: d_q'
        assert not bool(dqkv[:, :, C:2 * C].any()), f'{what}: d_k'
        assert not bool(dtab.any()), f'{what}: d_table'
        assert not bool(dqb.any()), f'{what}: d_qkv_bias'


def test_unsupported_storage_is_refused(dev):
    """The MFMA variants take bf16 storage only; float32 is GE_ERR_UNSUPPORTED, not a silent other kernel."""
    r, tab = _routed((1, 7, 7, 3), 0, 8, False)
    for variant in (2, 3):
        with pytest.raises(RuntimeError, match='unsupported'):
            run_kernel(dev, r['qkv'], r['qkv_bias'], tab, r['go'], 7, 7, 3, 0, variant, torch.float32, backward=False)


# ================================================================================ b. the mask is additive
# amplitude 2 on MI355X, worst over the geometries (l2rel, max/scale): v2 out / d_qkv / d_qkv_bias 1.00, 1.00; v2 d_table 1.27, 1.24;
# v1 f32 out 1.43, 1.44; d_qkv 1.32, 1.33; d_qkv_bias 4.08, 4.77 (of 8e-7: under RTOL); d_table 1.52, 1.24
@pytest.mark.parametrize('geom', GEOMS)
def test_mask_is_additive(dev, geom):
    """Queries matched to a key of ANOTHER region.  At amplitude 8 the match scores 362 - 100 and still takes all the weight: a kernel that used
    -inf or skipped masked keys gives something else.  At amplitude 2 it scores 23 - 100 and loses: compared with the float64 reference (the
    oracle's semantics: the mask is added) under the model's budget."""
    B, H, W, nH = geom
    r, tab = _routed(geom, 3, 8, True)
    if geom == (1, 8, 15, 6):                   # every window's real tokens share one region (the others hold pads only): plain routing
        assert r['n_cross'] == 0
    else:
        assert r['n_cross'] > 0 and r['dv'] is None
    for variant, dt in RUNS:
        o, _, _, _ = run_kernel(dev, r['qkv'], r['qkv_bias'], tab, r['go'], H, W, nH, 3, variant, dt, backward=False)
        assert torch.equal(o, r['out']), f'variant {variant} {dt} {geom}: {int((o != r["out"]).sum())} elements differ from the other-region gather'
    r2, tab = _routed(geom, 3, 2, True)
    args = (r2['qkv'], r2['qkv_bias'], tab, r2['go'], H, W, nH, 3)
    ref = reference(*args)
    for variant, dt, arith in ((1, torch.float32, 'f32'), (2, torch.bfloat16, 'bf16')):
        got = run_kernel(dev, *args, variant, dt)
        check_budget(f'mask amplitude 2 {geom} v{variant}', got, ref, R.model(*args, SCALE, arith), arith == 'f32')


# ================================================================================ c. stress inputs against float64
# worst kernel / budget ratio on MI355X over the three geometries, (l2rel, max/scale):
#   case        v2 out, d_qkv, d_qkv_bias   v2 d_table      v1 f32 out     d_qkv          d_qkv_bias     d_table   (v1: floor RTOL / ATOL applies)
#   normal      1.00, 1.00                  1.24, 1.89      1.42, 1.69     1.40, 1.48     1.42, 1.25     1.60, 1.83
#   peaked      1.00, 1.00                  0.87, 0.87      1.93, 2.07     1.98, 2.90     4.78, 4.10     1.92, 2.11
#   k_offset    1.00, 1.00                  0.84, 0.84      2.65, 2.56     1.77, 1.98     3.14, 2.57     2.51, 3.38
#   v_offset    1.00, 1.00                  1.18, 1.55      1.36, 1.51     2.11, 3.96     2.24, 3.01     2.23, 4.18
#   big_table   1.00, 1.00                  1.12, 1.52      1.15, 1.00     1.18, 1.46     1.09, 1.22     1.17, 1.26
#   all         1.00, 1.01                  1.01, 1.09      1.18, 2.36     1.05, 1.48     0.78, 0.66     1.09, 1.15
STRESS = ['normal', 'peaked', 'k_offset', 'v_offset', 'big_table', 'all']
STRESS_GEOMS = [((1, 8, 15, 6), 3),        # pads and shift
                ((1, 14, 21, 24), 0),      # no pads, nH = 24
                ((1, 14, 21, 24), 3)]      # masks without pads, nH = 24


def stress_inputs(geom, shift, case):
    """Storage-rounded (bf16-exact) inputs in float64.  peaked: q and k times 4; k_offset: +8 on every k channel, pad keys included, which cancels
    in exact arithmetic and tests the max-subtraction; v_offset: v + 30; big_table: table times 16."""
    B, H, W, nH = geom
    C = nH * 32
    g = gen(H * 100 + W + shift)
    qkv = torch.randn(B, H * W, 3 * C, generator=g, dtype=torch.float64)
    qb = 0.3 * torch.randn(3 * C, generator=g, dtype=torch.float64)
    tab = 0.5 * torch.randn(169, nH, generator=g, dtype=torch.float64)
    go = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
    if case in ('peaked', 'all'):
        qkv[:, :, :2 * C] *= 4
        qb[:2 * C] *= 4
    if case in ('k_offset', 'all'):
        qkv[:, :, C:2 * C] += 8
        qb[C:2 * C] += 8
    if case in ('v_offset', 'all'):
        qkv[:, :, 2 * C:] += 30
        qb[2 * C:] += 30
    if case in ('big_table', 'all'):
        tab *= 16
    return bf16_exact(qkv), bf16_exact(qb), tab.float().double(), bf16_exact(go)


@pytest.mark.parametrize('case', STRESS)
@pytest.mark.parametrize('geom,shift', STRESS_GEOMS)
def test_stress_against_float64(dev, geom, shift, case):
    """Variant 2 (bf16) and variant 1 (f32), forward and all four gradients, against the float64 reference (held to the oracle by
    test_winattn_ref_cpu.py) on the same storage-rounded inputs."""
    B, H, W, nH = geom
    args = stress_inputs(geom, shift, case) + (H, W, nH, shift)
    ref = reference(*args)
    for variant, dt, arith in ((2, torch.bfloat16, 'bf16'), (1, torch.float32, 'f32')):
        got = run_kernel(dev, *args, variant, dt)
        check_budget(f'{case} {geom} shift {shift} v{variant}', got, ref, R.model(*args, SCALE, arith), arith == 'f32')


# ================================================================================ d. many windows per workgroup
MANY = (3, 57, 63, 24)          # 243 windows over 64 persistent workgroups per head: some visit 3 windows, some 4
MANY_HEADS = (0, 23)
# on MI355X (l2rel, max/scale): v2 out / d_qkv / d_qkv_bias 1.00, 1.00; v2 d_table 0.83, 0.70; v1 f32 out 1.43, 0.99; d_qkv 1.37, 0.98; d_qkv_bias 1.25, 1.10;
# d_table 1.55, 1.68


@functools.lru_cache(maxsize=None)
def _many_inputs():
    B, H, W, nH = MANY
    C = nH * 32
    g = gen(57)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).bfloat16()
    qb = (0.3 * torch.randn(3 * C, generator=g)).bfloat16()
    tab = 0.5 * torch.randn(169, nH, generator=g)
    go = torch.randn(B, H * W, C, generator=g).bfloat16()
    return qkv, qb, tab, go


def test_many_windows_routing_and_repeatability(dev):
    """Routed inputs at the MANY geometry, bit for bit, on variants 1 (bf16) and 2: a persistent workgroup walks 3 or 4 windows with the token
    tables of two of them in LDS, and a dK / dV tile stored through another window's table lands in wrong rows, which fails the gathers exactly.

    Then variant 2 three times on the same inputs, the routed ones and the random ones of test_many_windows_per_workgroup (on the routed ones
    d_table and d_qkv_bias are zero): d_qkv is written by plain stores, d_table and d_qkv_bias are summed in a fixed order (per wave in LDS, then
    the two-stage reduction over workgroups), so all three are bit-identical from run to run.  Measured on MI355X before asserting: identical on
    both inputs, with this kernel and with its predecessor."""
    B, H, W, nH = MANY
    shift, C = 3, nH * 32
    r, tab = _routed(MANY, shift, 8, False)
    for variant, dt in ((1, torch.bfloat16), (2, torch.bfloat16)):
        what = f'variant {variant} {dt} {MANY} shift {shift}'
        o, dqkv, dqb, dtab = run_kernel(dev, r['qkv'], r['qkv_bias'], tab, r['go'], H, W, nH, shift, variant, dt)
        for x in (o, dqkv, dqb, dtab):
            assert bool(torch.isfinite(x).all()), what
        assert torch.equal(o, r['out']), f'{what}: out is not the gather, {int((o != r["out"]).sum())} elements differ'
        assert torch.equal(dqkv[:, :, 2 * C:], r['dv']), f'{what}: d_v is not the inverse gather, {int((dqkv[:, :, 2 * C:] != r["dv"]).sum())} elements differ'
        assert not bool(dqkv[:, :, :C].any()), f'{what}: d_q'
        assert not bool(dqkv[:, :, C:2 * C].any()), f'{what}: d_k'
        assert not bool(dtab.any()), f'{what}: d_table'
        assert not bool(dqb.any()), f'{what}: d_qkv_bias'
    for label, args in (('routed', (r['qkv'], r['qkv_bias'], tab, r['go'])), ('random', _many_inputs())):
        runs = [run_kernel(dev, *args, H, W, nH, shift, 2, torch.bfloat16) for _ in range(3)]
        same = {name: all(torch.equal(runs[0][i], x[i]) for x in runs[1:]) for i, name in enumerate(NAMES)}
        print(f'[winattn repeat {label} {MANY}] bit-identical over 3 runs: ' + ', '.join(f'{k} {v}' for k, v in same.items()))
        assert same['d_qkv'], f'{label}: d_qkv differs between runs on the same inputs'
        assert same['d_qkv_bias'] and same['d_table'], f'{label}: {same}'


def test_many_windows_per_workgroup(dev):
    """bwd_wg_per_head takes its ``want`` branch (Swin stage 0 at batch >= 3) and the windows do not divide evenly.  Heads are independent, so the
    float64 reference (oracle semantics) runs on heads 0 and 23 only: a 2-head problem on their columns, which test_winattn_ref_cpu.py shows
    equal to core(heads=(0, 23))."""
    from gedepth_amd import hip
    B, H, W, nH = MANY
    shift, C = 3, nH * 32
    n_bw = B * -(-H // 7) * -(-W // 7)
    wg_per_head = int(hip.lib().ge_window_attn_bwd_workspace(B, H, W, nH)) // (nH * (169 + 64) * 4)
    assert wg_per_head < -(-n_bw // 3), 'the workgroup count is capped by min_win, not by the resident-workgroup target'
    assert n_bw % wg_per_head != 0 and n_bw // wg_per_head >= 3, (n_bw, wg_per_head)
    qkv, qb, tab, go = _many_inputs()
    heads, cols = R.columns(nH, MANY_HEADS)
    sub = (qkv[:, :, cols].double(), qb[cols].double(), tab[:, heads].double(), go[:, :, cols[:len(cols) // 3]].double(), H, W, len(heads), shift)
    ref = reference(*sub)
    for variant, dt, arith in ((2, torch.bfloat16, 'bf16'), (1, torch.float32, 'f32')):
        o, dqkv, dqb, dtab = run_kernel(dev, qkv, qb, tab, go, H, W, nH, shift, variant, dt)
        got = (o[:, :, cols[:len(cols) // 3]], dqkv[:, :, cols], dqb[cols], dtab[:, heads])
        check_budget(f'many windows {MANY} heads {MANY_HEADS} v{variant}', got, ref, R.model(*sub, SCALE, arith), arith == 'f32')


# ================================================================================ e. fp8 edges
@pytest.mark.parametrize('which', ['q', 'v'])
def test_fp8_zero_tile(dev, which):
    """One (window, head) whose q (or v) is all zero, the pad bias included: tile_fp8_scale must not divide by an amax of 0.  The output is
    finite and equals variant 2's on that tile within the fp8 bound of test_window_attention_fp8_forward (12 % of the scale, here the tile's own).
    A zero v tile gives exactly 0 in both."""
    B, H, W, nH, shift = 2, 11, 20, 6, 3
    C = nH * 32
    g = gen(5)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).bfloat16()
    qb = (0.3 * torch.randn(3 * C, generator=g)).bfloat16()
    tab = 0.5 * torch.randn(169, nH, generator=g)
    tok, _ = R.tables(H, W, shift)
    b, win, head = 1, tok.shape[0] - 1, 4                          # the last window: it holds pad tokens
    assert bool((tok[win] < 0).any()) and bool((tok[win] >= 0).any())
    real = tok[win][tok[win] >= 0]
    part = {'q': 0, 'v': 2}[which]
    c0 = part * C + head * 32
    qkv[b, real, c0:c0 + 32] = 0
    qb[c0:c0 + 32] = 0
    o8, _, _, _ = run_kernel(dev, qkv, qb, tab, None, H, W, nH, shift, 3, torch.bfloat16, backward=False)
    o16, _, _, _ = run_kernel(dev, qkv, qb, tab, None, H, W, nH, shift, 2, torch.bfloat16, backward=False)
    assert bool(torch.isfinite(o8).all())
    t8, t16 = o8[b, real, head * 32:(head + 1) * 32], o16[b, real, head * 32:(head + 1) * 32]
    scale = t16.abs().max().item()
    err = (t8 - t16).abs().max().item()
    print(f'[winattn fp8 zero {which} tile] max err {err:.3e}, tile scale {scale:.3e}')
    assert err <= 0.12 * scale
    if which == 'v':
        assert scale == 0 and not bool(t8.any())
    else:
        assert scale > 0
