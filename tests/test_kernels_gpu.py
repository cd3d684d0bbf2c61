"""Parity of every HIP kernel (through the C ABI / autograd wrappers) against the CPU oracle, the
golden fixtures generated from the reference, and size-independent properties.  Runs on MI355X only."""
import json
import os

import numpy as np
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import gedepth_oracle as O
from oracle.fill import fill_state_dict

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5        # fp32: BASELINE.json north_star "within 1e-4 rel fp32"


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()                   # fail loudly if the native library is missing
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rtol=RTOL, atol=ATOL, what=''):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = ~(err <= tol)                      # a NaN / infinite error is not <= tol: a non-finite product value where the reference is finite fails
    nonfinite = int((~torch.isfinite(a)).sum())
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())}/{bad.numel()} off ({nonfinite} non-finite); max abs err {err.nan_to_num(nan=float("inf")).max():.3e} '
                                 f'(ref scale {b.abs().max():.3e})')


def close_scaled(a, b, rel=1e-4, what=''):
    """Gradient comparison: error relative to the tensor's max magnitude."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f'{what}: max abs err {err:.3e} vs scale {scale:.3e}'


def l2rel(a, b):
    """|a - b|_2 / |b|_2 in float64: unlike max-abs / scale it also holds the small-magnitude elements to account."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ====================================================================== window attention
def _attn_weights(C, nH, salt='t'):
    names = [('a.w_msa.relative_position_bias_table', (169, nH)), ('a.w_msa.qkv.weight', (3 * C, C)),
             ('a.w_msa.qkv.bias', (3 * C,)), ('a.w_msa.proj.weight', (C, C)), ('a.w_msa.proj.bias', (C,))]
    return fill_state_dict(names, salt)


def _product_attn(C, nH, shift, P, dev, variant=0):
    from gedepth_amd.depth.models.backbones.depthformer_swin import ShiftWindowMSA
    m = ShiftWindowMSA(C, nH, 7, shift_size=shift, dropout_layer=dict(type='DropPath', drop_prob=0.))
    m.load_state_dict({k[2:]: v for k, v in P.items()}, strict=False)
    m.kernel_variant = variant
    return m.to(dev)


@pytest.mark.parametrize('hw', [(11, 35), (10, 9), (14, 14), (7, 7), (3, 5)])
@pytest.mark.parametrize('shift', [0, 3])
def test_window_attention_fp32_fwd_bwd(dev, hw, shift):
    C, nH, B = 96, 3, 2
    H, W = hw
    P = _attn_weights(C, nH)
    x = torch.randn(B, H * W, C, generator=gen(H * 100 + W + shift))
    go = torch.randn(B, H * W, C, generator=gen(7))
    # oracle (CPU autograd)
    Pc = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xc = x.clone().requires_grad_(True)
    ref = O.shift_window_msa(xc, hw, Pc, 'a', nH, shift)
    ref.backward(go)
    # product (HIP)
    m = _product_attn(C, nH, shift, P, dev, variant=1)
    xg = x.to(dev).requires_grad_(True)
    out = m(xg, hw)
    out.backward(go.to(dev))
    close(out, ref, what='out')
    close_scaled(xg.grad, xc.grad, what='dx')
    close_scaled(m.w_msa.qkv.weight.grad, Pc['a.w_msa.qkv.weight'].grad, what='dWqkv')
    close_scaled(m.w_msa.qkv.bias.grad, Pc['a.w_msa.qkv.bias'].grad, what='dbqkv (incl. pad tokens)')
    close_scaled(m.w_msa.relative_position_bias_table.grad, Pc['a.w_msa.relative_position_bias_table'].grad,
                 what='d bias table')


@pytest.mark.parametrize('tag,hw', [('a', (11, 35)), ('b', (10, 9))])
@pytest.mark.parametrize('shift', [0, 3])
def test_window_attention_golden(dev, golden, tag, hw, shift):
    """Directly against outputs of the reference's ShiftWindowMSA (tests/golden/shift_window_msa.npz)."""
    g = golden('shift_window_msa')
    spec = json.loads(str(g['spec']))
    P = {'a.' + k: v for k, v in fill_state_dict([(n, s) for n, s in spec], 'shift_window_msa').items()}
    m = _product_attn(96, 3, shift, P, dev, variant=1)
    out = m(T(g[f'x_{tag}{shift}']).to(dev), hw)
    close(out, g[f'out_{tag}{shift}'], what='vs reference')


@pytest.mark.parametrize('shift', [0, 3])
def test_window_attention_bf16_storage(dev, shift):
    """bf16 storage / fp32 accumulate: compare with the oracle evaluated on the bf16-rounded qkv."""
    from gedepth_amd.kernels import window_attention
    B, H, W, nH = 2, 11, 20, 6
    C = nH * 32
    qkv = torch.randn(B, H * W, 3 * C, generator=gen(3)).bfloat16()
    qb = (0.1 * torch.randn(3 * C, generator=gen(4)))
    tab = 0.5 * torch.randn(169, nH, generator=gen(5))
    go = torch.randn(B, H * W, C, generator=gen(6)).bfloat16()

    def run(dt, variant):
        q = qkv.to(dev).to(dt).requires_grad_(True)
        b = qb.to(dev).requires_grad_(True)
        t = tab.to(dev).requires_grad_(True)
        o = window_attention(q, b if dt == torch.float32 else b, t, H, W, nH, shift, 32 ** -0.5, variant)
        o.backward(go.to(dev).to(dt))
        return o.float(), q.grad.float(), b.grad, t.grad

    # fp32 run on the same (bf16-representable) inputs, pad value rounded the same way
    qb_r = qb.bfloat16().float()
    q32 = qkv.float().to(dev).requires_grad_(True)
    b32 = qb_r.to(dev).requires_grad_(True)
    t32 = tab.to(dev).requires_grad_(True)
    o32 = window_attention(q32, b32, t32, H, W, nH, shift, 32 ** -0.5, 1)
    o32.backward(go.float().to(dev))
    o, dq, db, dt_ = run(torch.bfloat16, 1)
    close(o, o32, rtol=1e-2, atol=1e-2, what='bf16 out')
    close_scaled(dq, q32.grad, rel=2e-2, what='bf16 dqkv')
    close_scaled(dt_, t32.grad, rel=1e-3, what='bf16 dtable')
    close_scaled(db, b32.grad, rel=1e-3, what='bf16 dbias')


@pytest.mark.parametrize('geom', [(2, 11, 20, 6), (1, 14, 14, 3), (2, 3, 5, 3), (1, 22, 70, 12), (3, 7, 7, 24)])
@pytest.mark.parametrize('shift', [0, 3])
def test_window_attention_mfma_vs_exact(dev, geom, shift):
    """bf16 MFMA tile kernel (variant 2) against the exact-fp32 kernel evaluated on the same bf16-rounded inputs,
    forward and all four gradients (d_qkv, pad-token bias grad, bias-table grad)."""
    from gedepth_amd.kernels import window_attention
    B, H, W, nH = geom
    C = nH * 32
    g = gen(B * 1000 + H * 10 + W + shift)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).bfloat16()
    qb = (0.3 * torch.randn(3 * C, generator=g)).bfloat16().float()
    tab = 0.5 * torch.randn(169, nH, generator=g)
    go = torch.randn(B, H * W, C, generator=g).bfloat16()

    def run(dt, variant):
        q = qkv.to(dev).to(dt).requires_grad_(True)
        b = qb.to(dev).requires_grad_(True)
        t = tab.to(dev).requires_grad_(True)
        o = window_attention(q, b, t, H, W, nH, shift, 32 ** -0.5, variant)
        o.backward(go.to(dev).to(dt))
        return o.float(), q.grad.float(), b.grad, t.grad

    o_ref, dq_ref, db_ref, dt_ref = run(torch.float32, 1)
    o, dq, db, dtab = run(torch.bfloat16, 2)
    close(o, o_ref, rtol=2e-2, atol=2e-2, what='mfma out')
    close_scaled(dq, dq_ref, rel=2e-2, what='mfma dqkv')
    close_scaled(dtab, dt_ref, rel=1e-2, what='mfma d bias table')
    close_scaled(db, db_ref, rel=1e-2, what='mfma d qkv bias (pad tokens)')
    # mean error must be at bf16 rounding level, not just the max
    assert (o - o_ref).abs().mean().item() < 4e-3 * o_ref.abs().mean().item() + 1e-4
    assert (dq - dq_ref).abs().mean().item() < 6e-3 * dq_ref.abs().mean().item() + 1e-5


@pytest.mark.parametrize('geom,shift', [((2, 11, 35, 3), 0), ((2, 11, 35, 3), 3), ((1, 22, 70, 12), 3), ((2, 10, 9, 6), 0)])
def test_window_attention_fp8_forward(dev, geom, shift):
    """BASELINE.json configs[4]: the fp8 (OCP e4m3) MFMA forward (variant 3: QK^T and PV on v_mfma_f32_32x32x16_fp8_fp8, per
    (window, head) operand scales 448 / amax, probabilities as P * 256) against the exact-fp32 kernel on the same
    bf16-rounded inputs.  TOLERANCE RESTATED for fp8: e4m3 keeps 3 mantissa bits (relative step 2^-3 at worst, 2^-4 typ.):
    scores carry ~2^-4 * |q||k| noise averaged over 32 products and the softmax-weighted sum over <= 49 keys, which leaves
    the output within 1.2e-1 of its scale at worst and 6e-2 of the mean magnitude on average — measured on MI355X: max
    7.4e-2..8.9e-2, mean 4.3e-2..4.8e-2 for N(0,1) inputs, where the amax-scaled e4m3 grid is coarsest (bf16 MFMA: max 4e-3).  The backward is the bf16
    MFMA kernel's (gradients of the bf16 function at the same inputs) and is checked against variant 2 bit for bit."""
    from gedepth_amd.kernels import window_attention
    B, H, W, nH = geom
    C = nH * 32
    g = gen(B * 1000 + H * 10 + W + shift + 5)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).bfloat16()
    qb = (0.3 * torch.randn(3 * C, generator=g)).bfloat16().float()
    tab = 0.5 * torch.randn(169, nH, generator=g)
    go = torch.randn(B, H * W, C, generator=g).bfloat16()

    def run(dt, variant):
        q = qkv.to(dev).to(dt).requires_grad_(True)
        b = qb.to(dev).requires_grad_(True)
        t = tab.to(dev).requires_grad_(True)
        o = window_attention(q, b, t, H, W, nH, shift, 32 ** -0.5, variant)
        o.backward(go.to(dev).to(dt))
        return o.float(), q.grad.float(), b.grad, t.grad
    o_ref, _, _, _ = run(torch.float32, 1)
    o8, dq8, db8, dt8 = run(torch.bfloat16, 3)
    o16, dq16, db16, dt16 = run(torch.bfloat16, 2)
    scale = o_ref.abs().max().item()
    err = (o8 - o_ref).abs()
    print(f'\nfp8 forward {geom} shift {shift}: max err {err.max().item() / scale:.3e} of scale, mean {err.mean().item() / o_ref.abs().mean().item():.3e}; '
          f'bf16 MFMA: max {(o16 - o_ref).abs().max().item() / scale:.3e}')
    assert err.max().item() <= 0.12 * scale, err.max().item() / scale
    assert err.mean().item() <= 6e-2 * o_ref.abs().mean().item() + 1e-4
    assert err.mean().item() > (o16 - o_ref).abs().mean().item()            # it really is the lower-precision path
    assert torch.equal(dq8, dq16) and torch.equal(db8, db16) and torch.equal(dt8, dt16)


def test_window_attention_mfma_default_for_bf16(dev):
    """variant 0 (auto) must pick the MFMA kernel for bf16 storage and agree with it bit-for-bit."""
    from gedepth_amd.kernels import window_attention
    g = gen(77)
    qkv = torch.randn(2, 14 * 21, 3 * 96, generator=g).bfloat16().to(dev)
    qb, tab = torch.randn(288, generator=g).to(dev), torch.randn(169, 3, generator=g).to(dev)
    a = window_attention(qkv, qb, tab, 14, 21, 3, 3, 32 ** -0.5, 0)
    b = window_attention(qkv, qb, tab, 14, 21, 3, 3, 32 ** -0.5, 2)
    assert torch.equal(a, b)


def test_window_attention_pad_tokens_are_live(dev):
    """attention over an 11-row map == attention over the same map zero-extended to 14 rows
    (pad tokens act as keys/values equal to the qkv bias, they are not masked)."""
    C, nH = 96, 3
    P = _attn_weights(C, nH)
    for shift in (0, 3):
        m = _product_attn(C, nH, shift, P, dev, variant=1)
        x = torch.randn(1, 11 * 35, C, generator=gen(9)).to(dev)
        x14 = torch.cat([x.view(1, 11, 35, C), torch.zeros(1, 3, 35, C, device=dev)], 1).view(1, 14 * 35, C)
        a = m(x, (11, 35))
        b = m(x14, (14, 35)).view(1, 14, 35, C)[:, :11].reshape(1, 11 * 35, C)
        assert torch.equal(a, b)


# ================================================================================== MSDA
def _msda_inputs(seed, B=2, Nq=70, shapes=((11, 35), (6, 18), (3, 9), (2, 5))):
    g = gen(seed)
    nv = sum(h * w for h, w in shapes)
    value = torch.randn(B, nv, 8, 64, generator=g)
    loc = torch.rand(B, Nq, 8, 4, 8, 2, generator=g) * 1.3 - 0.15        # includes out-of-range samples
    aw = torch.rand(B, Nq, 8, 4, 8, generator=g).flatten(-2).softmax(-1).view(B, Nq, 8, 4, 8)
    go = torch.randn(B, Nq, 512, generator=g)
    return value, loc, aw, go, [tuple(s) for s in shapes]


@pytest.mark.parametrize('binned', [True, False])
@pytest.mark.parametrize('shapes', [((11, 35), (6, 18), (3, 9), (2, 5)), ((40, 70), (20, 35), (10, 18), (5, 9))])
def test_msda_fp32_fwd_bwd(dev, binned, shapes, monkeypatch):
    """binned=True: count/scan/fill/drain scatter (one integer atomic per tap); False: fp32 atomic bursts."""
    from gedepth_amd import kernels
    from gedepth_amd.kernels import ms_deform_attn
    monkeypatch.setattr(kernels, 'MSDA_BINNED_BACKWARD', binned)
    value, loc, aw, go, shapes = _msda_inputs(1, B=2, Nq=300 if shapes[0][0] == 40 else 70, shapes=shapes)
    vc, lc, ac = (t.clone().requires_grad_(True) for t in (value, loc, aw))
    ref = O.msda_core(vc, shapes, lc, ac)
    ref.backward(go)
    vg, lg, ag = (t.to(dev).requires_grad_(True) for t in (value, loc, aw))
    out = ms_deform_attn(vg, shapes, lg, ag)
    out.backward(go.to(dev))
    close(out, ref, what='out')
    close_scaled(vg.grad, vc.grad, what='d value')
    close_scaled(ag.grad, ac.grad, what='d attw')
    close_scaled(lg.grad, lc.grad, rel=2e-4, what='d loc')


def _coherent_locations(B, qshapes, shapes, seed, spread=0.0, jitter=2.5):
    """Sampling locations like the HAHI neck produces: reference point = the query's own (normalised) pixel centre, offsets
    of a few pixels of each level; ``spread`` adds a fraction of scattered points (anywhere, incl. outside the map)."""
    g = gen(seed)
    refs = []
    for h, w in qshapes:
        gy, gx = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        refs.append(torch.stack((gx.reshape(-1), gy.reshape(-1)), -1))
    ref = torch.cat(refs, 0)                                              # (Nq, 2)
    Nq = ref.shape[0]
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)   # (L, 2)
    off = jitter * torch.randn(B, Nq, 8, len(shapes), 8, 2, generator=g)
    loc = ref[None, :, None, None, None, :] + off / norm[None, None, None, :, None, :]
    if spread > 0:
        wild = torch.rand(B, Nq, 8, len(shapes), 8, 1, generator=g) < spread
        loc = torch.where(wild, torch.rand(loc.shape, generator=g) * 1.4 - 0.2, loc)
    aw = torch.rand(B, Nq, 8, len(shapes), 8, generator=g).flatten(-2).softmax(-1).view(B, Nq, 8, len(shapes), 8)
    return loc, aw


@pytest.mark.parametrize('case', ['self', 'cross', 'scattered', 'ragged'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_msda_window_kernels(dev, case, dtype):
    """The LDS-window kernels (csrc/msda_win.hip: 2-D query tiles, per-(tile, level) staged value windows, global
    fallback when a window does not fit) against the CPU oracle (fp32) and against the streaming kernels (both dtypes):
    forward, d_loc, d_attw, d_value.  'self': queries = the levels themselves; 'cross': one query map at twice the
    resolution of level 0; 'scattered': uniformly random locations (every finest-level window overflows -> fallback
    path); 'ragged': map sizes that are not multiples of the tile, 5 % scattered points, a level smaller than a tile."""
    from gedepth_amd.kernels import ms_deform_attn, msda_mode
    shapes = {'self': ((44, 70), (22, 35), (11, 18), (6, 9)), 'cross': ((22, 35), (11, 18), (6, 9), (3, 5)),
              'scattered': ((44, 70), (22, 35), (11, 18), (6, 9)), 'ragged': ((37, 53), (19, 27), (10, 14), (5, 7))}[case]
    qshapes = {'self': shapes, 'cross': ((44, 70),), 'scattered': shapes, 'ragged': ((21, 45), (3, 5))}[case]
    B = 2
    nv = sum(h * w for h, w in shapes)
    nq = sum(h * w for h, w in qshapes)
    g = gen(17)
    value = torch.randn(B, nv, 8, 64, generator=g)
    go = torch.randn(B, nq, 512, generator=g)
    if case == 'scattered':
        loc = torch.rand(B, nq, 8, 4, 8, 2, generator=g) * 1.3 - 0.15
        aw = torch.rand(B, nq, 8, 4, 8, generator=g).flatten(-2).softmax(-1).view(B, nq, 8, 4, 8)
    else:
        loc, aw = _coherent_locations(B, qshapes, shapes, 5, spread=0.05 if case == 'ragged' else 0.0)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    value, go = value.to(td), go.to(td)

    def run(mode, qs):
        old = msda_mode(mode)
        try:
            vg = value.to(dev).requires_grad_(True)
            lg, ag = loc.to(dev).requires_grad_(True), aw.to(dev).requires_grad_(True)
            out = ms_deform_attn(vg, shapes, lg, ag, query_shapes=qs)
            out.backward(go.to(dev))
            return [t.float().cpu() for t in (out, vg.grad, lg.grad, ag.grad)]
        finally:
            msda_mode(old)
    win = run(7, qshapes)                                   # window kernels (forward + d_loc/d_attw), owner-lane tap arithmetic
    win_plain = run(3, qshapes)                             # window kernels, per-lane tap arithmetic
    stream = run(0, qshapes)
    stream_hm = run(8, qshapes)                             # streaming kernels, head-major work order
    mix = run(13, qshapes)                                  # window forward, streaming head-major backward, VALU drain
    default = run(61, qshapes)                              # the default: the same + bf16 d_value drain on MFMA (transposing LDS reads), chunks drained in bin order
    grouped = run(125, qshapes)                             # + drain work order grouped by query range (msda_order_k, opt-in)
    mfma_plain = run(29, qshapes)                           # MFMA drain with plain 16-bit LDS reads for the B operand
    names = ('out', 'd value', 'd loc', 'd attw')
    # same arithmetic per (query, head): the decompositions agree to the order of the 8-lane / 16-lane reductions
    for w, tag in ((win, 'window'), (win_plain, 'window (per-lane taps)'), (stream_hm, 'streaming head-major'), (mix, 'mode 13'),
                   (default, 'default mode 61'), (grouped, 'mode 125'), (mfma_plain, 'mode 29')):
        for a, b, n in zip(w, stream, names):
            if dtype == 'f32':
                close_scaled(a, b, rel=2e-5, what=f'{tag} vs streaming: {n}')
            else:
                close_scaled(a, b, rel=1e-2 if n in ('out', 'd value') else 2e-5, what=f'{tag} vs streaming (bf16): {n}')
    if dtype == 'f32':
        vc, lc, ac = (t.clone().requires_grad_(True) for t in (value, loc, aw))
        ref = O.msda_core(vc, shapes, lc, ac)
        ref.backward(go)
        close(win[0], ref, what='out vs oracle')
        close_scaled(win[1], vc.grad, what='d value vs oracle')
        close_scaled(win[3], ac.grad, what='d attw vs oracle')
        close_scaled(win[2], lc.grad, rel=2e-4, what='d loc vs oracle')


def test_msda_large_maps_use_per_head_histograms(dev):
    """Value maps with thousands of tiles (native-resolution DDAD, config #4): the counting sort's work units hold one head's
    tiles in LDS (a histogram over all heads would not fit); same results as the oracle, and the workspace path is really taken."""
    from gedepth_amd import hip, kernels
    from gedepth_amd.kernels import ms_deform_attn
    import ctypes
    shapes = ((200, 320), (100, 160), (50, 80), (25, 40))                  # 2665 tiles x 8 heads x 4 B = 85 KB > 60 KB
    value, loc, aw, go, shapes = _msda_inputs(3, B=1, Nq=90, shapes=shapes)
    arr = (ctypes.c_int * 8)(*[v for hw in shapes for v in hw])
    Nv = sum(h * w for h, w in shapes)
    assert hip.lib().ge_msda_bwd_workspace(ctypes.cast(arr, ctypes.c_void_p), 1, Nv, 90, 8, 4, 8) > 0
    vc, lc, ac = (t.clone().requires_grad_(True) for t in (value, loc, aw))
    ref = O.msda_core(vc, shapes, lc, ac)
    ref.backward(go)
    vg, lg, ag = (t.to(dev).requires_grad_(True) for t in (value, loc, aw))
    kernels.PROFILER.enable()
    out = ms_deform_attn(vg, shapes, lg, ag)
    out.backward(go.to(dev))
    kernels.PROFILER.disable()
    assert any(r['name'] == 'msda_drain_k' for r in kernels.PROFILER.msda_bwd_stages())       # the binned path ran
    close(out, ref, what='out')
    close_scaled(vg.grad, vc.grad, what='d value')
    close_scaled(ag.grad, ac.grad, what='d attw')
    close_scaled(lg.grad, lc.grad, rel=2e-4, what='d loc')


def test_msda_golden(dev, golden):
    from gedepth_amd.kernels import ms_deform_attn
    g = golden('msda_core')
    shapes = [tuple(int(v) for v in s) for s in g['shapes']]
    out = ms_deform_attn(T(g['value']).to(dev), shapes, T(g['loc']).to(dev), T(g['aw']).to(dev))
    close(out, g['out'], what='vs mmcv-semantics fixture')


def test_msda_bf16(dev):
    from gedepth_amd.kernels import ms_deform_attn
    value, loc, aw, go, shapes = _msda_inputs(2)
    vb = value.bfloat16()
    ref = O.msda_core(vb.float(), shapes, loc, aw)
    vg = vb.to(dev).requires_grad_(True)
    lg, ag = loc.to(dev).requires_grad_(True), aw.to(dev).requires_grad_(True)
    out = ms_deform_attn(vg, shapes, lg, ag)
    assert out.dtype == torch.bfloat16
    close(out.float(), ref, rtol=1e-2, atol=1e-2, what='bf16 out')
    out.backward(go.bfloat16().to(dev))
    assert vg.grad.dtype == torch.bfloat16 and torch.isfinite(vg.grad.float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [125, 61, 29, 13, 64, 0, 8, 7])
@pytest.mark.parametrize('binned', [True, False])
def test_msda_bf16_gradients_vs_oracle(dev, mode, binned, monkeypatch):
    """bf16 storage path against the fp32 CPU oracle evaluated on the SAME bf16-rounded value / gradient rows: d_loc and d_attw are
    fp32 sums of bf16 products (exact up to summation order), d_value and out are rounded to bf16 once.  Covers the bf16-pair dot
    products (v_dot2) of the d_loc / d_attw kernels in every kernel-selection mode."""
    from gedepth_amd import kernels
    from gedepth_amd.kernels import ms_deform_attn, msda_mode
    monkeypatch.setattr(kernels, 'MSDA_BINNED_BACKWARD', binned)
    shapes = ((40, 70), (20, 35), (10, 18), (5, 9))
    qshapes = [(20, 35)]
    value, loc, aw, go, shapes = _msda_inputs(5, B=2, Nq=20 * 35, shapes=shapes)
    vb, gb = value.bfloat16(), go.bfloat16()
    vc, lc, ac = vb.float().requires_grad_(True), loc.clone().requires_grad_(True), aw.clone().requires_grad_(True)
    ref = O.msda_core(vc, shapes, lc, ac)
    ref.backward(gb.float())
    old = msda_mode(mode)
    try:
        vg = vb.to(dev).requires_grad_(True)
        lg, ag = loc.to(dev).requires_grad_(True), aw.to(dev).requires_grad_(True)
        out = ms_deform_attn(vg, shapes, lg, ag, query_shapes=qshapes)
        out.backward(gb.to(dev))
    finally:
        msda_mode(old)
    close_scaled(out.float(), ref, rel=1e-2, what='bf16 out')
    close_scaled(vg.grad.float(), vc.grad, rel=1e-2, what='bf16 d value')
    close_scaled(ag.grad, ac.grad, rel=2e-5, what='bf16 d attw')
    close_scaled(lg.grad, lc.grad, rel=2e-4, what='bf16 d loc')


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [125, 61, 29, 13, 77])
def test_msda_drain_many_records_per_tile(dev, mode):
    """d_value when a value tile collects far more than one chunk of records (4096): 4000 queries x 8 points land on a level of
    2 x 4 tiles, so every bin is drained by several waves whose partial tiles meet through fp32 atomics; the last block of a
    chunk is ragged.  bf16 storage: the MFMA drain (mode bit 4; bit 5 = ds_read_b64_tr_b16 operand reads) and the VALU drain
    against the fp32 oracle on the same bf16-rounded rows."""
    from gedepth_amd import kernels
    from gedepth_amd.kernels import ms_deform_attn, msda_mode
    shapes = ((8, 16), (4, 8), (2, 4), (1, 2))
    value, loc, aw, go, shapes = _msda_inputs(11, B=2, Nq=4001, shapes=shapes)
    vb, gb = value.bfloat16(), go.bfloat16()
    vc = vb.float().requires_grad_(True)
    ref = O.msda_core(vc, shapes, loc, aw)
    ref.backward(gb.float())
    old = msda_mode(mode)
    try:
        vg = vb.to(dev).requires_grad_(True)
        kernels.PROFILER.enable()
        out = ms_deform_attn(vg, shapes, loc.to(dev), aw.to(dev))
        out.backward(gb.to(dev))
        kernels.PROFILER.disable()
        stages = [r['name'] for r in kernels.PROFILER.msda_bwd_stages()]
    finally:
        msda_mode(old)
    assert ('msda_drain_mfma_k' if mode & 16 else 'msda_drain_k') in stages, stages
    close_scaled(vg.grad.float(), vc.grad, rel=1e-2, what=f'bf16 d value, mode {mode}')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('case', ['self', 'cross'])
def test_msda_raw_fused_prepare_and_sampling(dev, dtype, case):
    """kernels.ms_deform_attn_raw (ge_msda_fwd_raw / ge_msda_bwd_raw: view -> softmax -> normaliser -> reference points -> sampling
    in one kernel, and its backward straight to the raw projection gradient) against (1) mmcv's arithmetic written out in torch on
    the CPU with the oracle's sampling core, differentiated by autograd (fp32), and (2) the two-pass composition msda_prepare +
    ms_deform_attn on the GPU (both dtypes): out, d_value, d_raw (offsets and logits), d_ref.  'self': queries = the four levels
    (ragged tiles), reference = pixel centres; 'cross': one 2x query map, reference points requiring a gradient."""
    from gedepth_amd import hip
    from gedepth_amd.kernels import ms_deform_attn_raw, msda_mode
    shapes = [(22, 35), (11, 18), (6, 9), (3, 5)]
    qshapes = shapes if case == 'self' else [(44, 70)]
    B, nH, L, P = 2, 8, 4, 8
    nv = sum(h * w for h, w in shapes)
    nq = sum(h * w for h, w in qshapes)
    g = gen(23)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    value = torch.randn(B, nv, nH, 64, generator=g).to(td)
    raw = torch.cat((torch.randn(B, nq, nH * L * P * 2, generator=g) * 2.5, torch.randn(B, nq, nH * L * P, generator=g)), -1).to(td)
    refs = []
    for h, w in qshapes:
        gy, gx = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        refs.append(torch.stack((gx.reshape(-1), gy.reshape(-1)), -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(B, nq, L, 2).contiguous()
    if case == 'cross':
        ref = (ref + 0.02 * torch.randn(B, nq, L, 2, generator=g)).clamp(0.01, 0.99)
    go = torch.randn(B, nq, nH * 64, generator=g).to(td)

    def run(mode):
        old = msda_mode(mode)
        try:
            v, r, rf = value.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True), ref.to(dev).requires_grad_(True)
            out = ms_deform_attn_raw(v, r, rf, shapes, qshapes, nH, L, P)
            out.backward(go.to(dev))
            return [t.float().cpu() for t in (out, v.grad, r.grad, rf.grad)]
        finally:
            msda_mode(old)
    arr = (ctypes.c_int * 8)(*[x for hw in shapes for x in hw])
    qa = (ctypes.c_int * (2 * len(qshapes)))(*[x for hw in qshapes for x in hw])
    sup = hip.lib().ge_msda_raw_supported(ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(qa, ctypes.c_void_p), len(qshapes), B, nv, nq, nH, L, P)
    assert sup == 1                                            # the fused kernels are what `run(61)` exercises
    fused = run(61)
    composed = run(60)                                         # mode without the window forward: prepare pass + streaming kernels
    n_off = nH * L * P * 2
    names = ('out', 'd value', 'd raw', 'd ref')
    for a, b, n in zip(fused, composed, names):
        if dtype == 'f32':
            close_scaled(a, b, rel=3e-5, what=f'fused vs composed: {n}')
        else:                                                   # bf16: outputs / d_value / d_raw are rounded to bf16 once on either path
            close_scaled(a, b, rel=1e-2, what=f'fused vs composed (bf16): {n}')
    if dtype == 'f32':
        vc, rc, fc = value.clone().requires_grad_(True), raw.clone().requires_grad_(True), ref.clone().requires_grad_(True)
        off = rc[..., :n_off].view(B, nq, nH, L, P, 2)
        norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
        loc = fc[:, :, None, :, None, :] + off / norm
        aw = rc[..., n_off:].view(B, nq, nH, L * P).softmax(-1).view(B, nq, nH, L, P)
        o = O.msda_core(vc, shapes, loc, aw)
        o.backward(go)
        close(fused[0], o, what='out vs oracle')
        close_scaled(fused[1], vc.grad, what='d value vs oracle')
        close_scaled(fused[2][..., n_off:], rc.grad[..., n_off:], rel=2e-4, what='d logits vs oracle')
        close_scaled(fused[2][..., :n_off], rc.grad[..., :n_off], rel=2e-4, what='d offsets vs oracle')
        close_scaled(fused[3], fc.grad, rel=2e-4, what='d ref vs oracle')


# ---- deformable attention as MFMA contractions on LDS windows (csrc/msda_mm.hip, round 4)
def _mm_refs(qshapes):
    """Pixel-centre reference points, moved OFF the k/64 grid of bf16 offsets: a sample that lands exactly on a pixel sits on the kink
    of the bilinear gradient, where the last bit of the location decides which one-sided derivative d_offset gets."""
    r = []
    for h, w in qshapes:
        gy, gx = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        r.append(torch.stack((gx.reshape(-1) + 0.013 / w, gy.reshape(-1) + 0.017 / h), -1))
    return torch.cat(r, 0)


_MM_CASES = {
    # name: (value shapes, query shapes, offset scale in pixels, reference points, query order)
    'self-tiles': (((44, 70), (22, 35), (11, 18), (6, 9)), 'same', 2.5, 'grid', 'tile'),
    'self-identity': (((44, 70), (22, 35), (11, 18), (6, 9)), 'same', 2.5, 'grid', None),
    'cross-grid': (((22, 35), (11, 18), (6, 9), (3, 5)), ((44, 70),), 2.5, 'grid', 'tile'),
    'cross-sorted': (((44, 70), (22, 35), (11, 18), (6, 9)), ((37, 41),), 2.5, 'rand', 'ref'),
    'scattered': (((44, 70), (22, 35), (11, 18), (6, 9)), ((37, 41),), 6.0, 'rand', 'randperm'),      # windows of many chunks
    'ragged': (((37, 53), (19, 27), (10, 14), (5, 7)), ((21, 45), (3, 5)), 4.0, 'grid', 'tile'),          # Nq % 32 != 0
    'tiny': (((3, 5), (2, 3), (1, 2), (1, 1)), ((2, 3),), 1.0, 'grid', 'tile'),                          # one partial tile, 1 x 1 level
    # 36 super-blocks at level 0 and tiles without any locality: the value-stationary kernel hands (nearly) every tile to its atomic fallback
    'strays': (((88, 140), (44, 70), (22, 35), (11, 18)), ((37, 41),), 6.0, 'rand', 'randperm'),
}


@pytest.mark.parametrize('case', sorted(_MM_CASES))
def test_msda_mm_fwd_bwd_vs_oracle(dev, case):
    """kernels.ms_deform_attn_mm (ge_msda_fwd_mm / ge_msda_bwd_lw_mm / ge_msda_bwd_value / ge_msda_dref) against mmcv's arithmetic
    written out in torch on the CPU with the oracle's sampling core, differentiated by autograd, on the SAME bf16-rounded value /
    raw / gradient tensors: out, d_value, d_offsets, d_logits, d_reference_points.  Tolerance 1e-2 of each tensor's scale = one bf16
    rounding of the result (measured 2e-3 ... 6e-3).  The query order never changes the result."""
    from gedepth_amd import kernels as K
    shapes, qshapes, jitter, ref_mode, order_mode = _MM_CASES[case]
    qshapes = shapes if qshapes == 'same' else qshapes
    B, nH, L, P = 2, 8, 4, 8
    g = gen(sum(map(ord, case)))
    nv, nq = sum(h * w for h, w in shapes), sum(h * w for h, w in qshapes)
    n_off = nH * L * P * 2
    value = torch.randn(B, nv, nH, 64, generator=g).bfloat16()
    raw = torch.cat((torch.randn(B, nq, n_off, generator=g) * jitter, torch.randn(B, nq, nH * L * P, generator=g)), -1).bfloat16()
    ref = _mm_refs(qshapes) if ref_mode == 'grid' else torch.rand(nq, 2, generator=g) * 1.2 - 0.1       # incl. points outside the maps
    ref = ref[None, :, None, :].expand(B, nq, L, 2).contiguous()
    go = torch.randn(B, nq, nH * 64, generator=g).bfloat16()
    vc, rc, fc = value.float().requires_grad_(True), raw.float().requires_grad_(True), ref.clone().requires_grad_(True)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = fc[:, :, None, :, None, :] + rc[..., :n_off].view(B, nq, nH, L, P, 2) / norm
    aw = rc[..., n_off:].view(B, nq, nH, L * P).softmax(-1).view(B, nq, nH, L, P)
    want = O.msda_core(vc, shapes, loc, aw)
    want.backward(go.float())
    order = {'tile': lambda: K.msda_tile_order(qshapes, dev), 'ref': lambda: K.msda_ref_order(ref[0, :, 0].to(dev), shapes[0]),
             'randperm': lambda: torch.randperm(nq, generator=g).to(torch.int32).to(dev), None: lambda: None}[order_mode]()
    assert K.msda_mm_supported(value.to(dev), raw.to(dev), shapes, nH, L, P)
    v, r, f = value.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True), ref.to(dev).requires_grad_(True)
    out = K.ms_deform_attn_mm(v, r, f, shapes, order, nH, L, P)
    out.backward(go.to(dev))
    close_scaled(out.float(), want, rel=1e-2, what='out')
    close_scaled(v.grad.float(), vc.grad, rel=1e-2, what='d value')
    close_scaled(r.grad[..., :n_off].float(), rc.grad[..., :n_off], rel=1e-2, what='d offsets')
    close_scaled(r.grad[..., n_off:].float(), rc.grad[..., n_off:], rel=1e-2, what='d logits')
    close_scaled(f.grad, fc.grad, rel=1e-2, what='d reference points')
    # l2-relative (round-4 review: max-abs / scale leaves small elements unchecked).  bf16 results: one rounding = 2^-9 per element
    # -> ~1.6e-3 in l2; the coefficient image adds its own bf16 roundings
    l2 = dict(out=l2rel(out.float(), want), d_value=l2rel(v.grad.float(), vc.grad), d_offsets=l2rel(r.grad[..., :n_off].float(), rc.grad[..., :n_off]),
              d_logits=l2rel(r.grad[..., n_off:].float(), rc.grad[..., n_off:]))
    print(f'\n[msda mm {case}] l2-relative errors vs the fp32 oracle on bf16-rounded inputs: ' + ', '.join(f'{k} {e:.2e}' for k, e in l2.items()))
    assert all(e <= 5e-3 for e in l2.values()), l2
    # d_value comes from two kernels selected by a LEVEL MASK (kernels._MMValueChoice; the call above ran all levels through the record pipeline, the
    # choice's starting point since round 6): every split must give the same tensor — all levels on the MFMA kernel, coarse / fine and odd / even splits
    # ... and the value-stationary kernel (round 6, ge_msda_bwd_value_vs; 'randperm' / random reference points make most tiles STRAY: they take
    # its per-tile fallback to the atomic kernel, the grid cases the super-block lists)
    for mode in ('mm', '12', '5', '10', 'vs'):
        K._MM_VALUE_CHOICE.clear()
        os.environ['GE_MSDA_VALUE'] = mode
        try:
            v2, r2 = value.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True)
            K.ms_deform_attn_mm(v2, r2, ref.to(dev), shapes, order, nH, L, P).backward(go.to(dev))
        finally:
            os.environ.pop('GE_MSDA_VALUE', None)
            K._MM_VALUE_CHOICE.clear()
        close_scaled(v2.grad.float(), vc.grad, rel=1e-2, what=f'd value (GE_MSDA_VALUE={mode})')
        assert l2rel(v2.grad.float(), vc.grad) <= 5e-3, (mode, l2rel(v2.grad.float(), vc.grad))
        assert torch.equal(r2.grad, r.grad)
    # the same call in another order: identical up to the bf16 rounding of the coefficient sums (different tiles, different chunking)
    other = torch.arange(nq - 1, -1, -1, dtype=torch.int32, device=dev)
    out2 = K.ms_deform_attn_mm(v.detach(), r.detach(), f.detach(), shapes, other, nH, L, P)
    close_scaled(out2.float(), out.float(), rel=1e-2, what='reversed query order')


@pytest.mark.parametrize('shapes', [((44, 70), (22, 35), (11, 18), (6, 9)), ((37, 53), (19, 27), (10, 14), (5, 7))])
def test_msda_self_split_vs_oracle_and_window_kernels(dev, shapes):
    """kernels.ms_deform_attn_self_split (round 6): the self-attention's sampling with the level-0 queries on the MFMA kernels
    (ge_msda_fwd_mm_part / ge_msda_bwd_lw_mm_part: rows addressed in place through the row pitch) and the coarse-level queries on the window
    kernels, d_value from the record pipeline over all queries — against mmcv's arithmetic in torch on the CPU (oracle sampling core, autograd)
    on the same bf16-rounded tensors, and against the all-window path it replaces.  Second case: odd sizes, level-0 count not a multiple of 32."""
    from gedepth_amd import kernels as K
    B, nH, L, P = 2, 8, 4, 8
    g = gen(91 + shapes[0][0])
    nv = sum(h * w for h, w in shapes)
    n_off = nH * L * P * 2
    value = torch.randn(B, nv, nH, 64, generator=g).bfloat16()
    raw = torch.cat((torch.randn(B, nv, n_off, generator=g) * 2.5, torch.randn(B, nv, nH * L * P, generator=g)), -1).bfloat16()
    ref = _mm_refs(shapes)[None, :, None, :].expand(B, nv, L, 2).contiguous()
    go = torch.randn(B, nv, nH * 64, generator=g).bfloat16()
    vc, rc = value.float().requires_grad_(True), raw.float().requires_grad_(True)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref[:, :, None, :, None, :] + rc[..., :n_off].view(B, nv, nH, L, P, 2) / norm
    aw = rc[..., n_off:].view(B, nv, nH, L * P).softmax(-1).view(B, nv, nH, L, P)
    want = O.msda_core(vc, shapes, loc, aw)
    want.backward(go.float())
    assert K.msda_self_split_ok(value.to(dev), raw.to(dev), shapes, shapes, nH, L, P)
    res = {}
    for tag in ('split', 'window'):
        v, r = value.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True)
        refd = ref.to(dev)[:1].expand(B, nv, L, 2)                      # an expanded view, as the neck passes it
        out = K.ms_deform_attn_self_split(v, r, refd, shapes, nH, L, P) if tag == 'split' else K.ms_deform_attn_raw(v, r, refd, shapes, shapes, nH, L, P)
        out.backward(go.to(dev))
        res[tag] = (out.float().cpu(), v.grad.float().cpu(), r.grad.float().cpu())
        l2 = dict(out=l2rel(res[tag][0], want), d_value=l2rel(res[tag][1], vc.grad), d_offsets=l2rel(res[tag][2][..., :n_off], rc.grad[..., :n_off]),
                  d_logits=l2rel(res[tag][2][..., n_off:], rc.grad[..., n_off:]))
        print(f'\n[msda self {tag} {shapes[0]}] l2-relative errors vs the fp32 oracle on bf16-rounded inputs: ' + ', '.join(f'{k} {e:.2e}' for k, e in l2.items()))
        assert all(e <= 5e-3 for e in l2.values()), (tag, l2)
        close_scaled(res[tag][0], want, rel=1e-2, what=f'out ({tag})')
        close_scaled(res[tag][2][..., :n_off], rc.grad[..., :n_off], rel=1e-2, what=f'd offsets ({tag})')
    n0 = shapes[0][0] * shapes[0][1]
    # the coarse-level rows come from the SAME window kernels in both paths: identical bits; the level-0 rows differ by the two decompositions' roundings
    assert torch.equal(res['split'][0][:, n0:], res['window'][0][:, n0:]) and torch.equal(res['split'][2][:, n0:], res['window'][2][:, n0:])
    assert not torch.equal(res['split'][0][:, :n0], res['window'][0][:, :n0])
    close_scaled(res['split'][0], res['window'][0], rel=1e-2, what='split vs window out')


def test_msda_mm_cross_attention_shape_offset_gradient_vs_float64(dev):
    """Round-3 review, weak #1: the gradient of the cross-attention's ``sampling_offsets`` projection at config #3's real shape
    (2 images x 98 560 queries) was only asserted through a model-level cosine that moved between runs.  Here the op is isolated at
    that shape: d_raw of ge_msda_bwd_lw_mm against the oracle's sampling core in FLOAT64 on the same bf16-rounded value / raw /
    gradient rows, then contracted with a query matrix exactly as the Linear's weight gradient contracts it (dW = d_raw^T q over all
    197 120 tokens, float64 on both sides): the DIRECTION of that tensor is asserted (cosine), and so is run-to-run bit equality of
    d_raw (no atomics on this path) — noise and error can no longer be confused."""
    from gedepth_amd import kernels as K
    from gedepth_amd.mmrt.bricks import msda_offset_bias
    shapes = ((88, 280), (44, 140), (22, 70), (11, 35))
    B, nH, L, P = 2, 8, 4, 8
    nq, nv = 176 * 560, sum(h * w for h, w in shapes)
    n_off = nH * L * P * 2
    g = gen(41)
    value = torch.randn(B, nv, nH, 64, generator=g).bfloat16()
    raw = torch.cat((msda_offset_bias(nH, L, P)[None, None] + 0.3 * torch.randn(B, nq, n_off, generator=g),
                     0.5 * torch.randn(B, nq, nH * L * P, generator=g)), -1).bfloat16()
    ref = torch.sigmoid(torch.randn(nq, 2, generator=g))[None, :, None, :].expand(B, nq, L, 2).contiguous()     # content-independent, like hahi.py:294-302
    go = torch.randn(B, nq, nH * 64, generator=g).bfloat16()
    query = torch.randn(B * nq, 64, generator=g).bfloat16()           # 64 input features stand in for the 512 of the real Linear
    # float64 oracle (the sampling core on the CPU; ~1 minute)
    vc, rc = value.double().requires_grad_(True), raw.double().requires_grad_(True)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
    loc = ref.double()[:, :, None, :, None, :] + rc[..., :n_off].view(B, nq, nH, L, P, 2) / norm
    aw = rc[..., n_off:].view(B, nq, nH, L * P).softmax(-1).view(B, nq, nH, L, P)
    O.msda_core(vc, shapes, loc, aw).backward(go.double())
    want = rc.grad[..., :n_off].reshape(B * nq, n_off)
    order = K.msda_ref_order(ref[0, :, 0].to(dev), shapes[0])
    runs = []
    for _ in range(2):
        v, r = value.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True)
        K.ms_deform_attn_mm(v, r, ref.to(dev), shapes, order, nH, L, P).backward(go.to(dev))
        runs.append((r.grad.clone(), v.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]), 'd_raw must be bit-reproducible (no atomics on the d_loc / d_attw path)'
    dv_noise = (runs[0][1].float() - runs[1][1].float()).abs().max().item() / runs[0][1].float().abs().max().item()
    assert dv_noise <= 2 ** -7, dv_noise                               # d_value: fp32 atomics between chunk partials, then one bf16 rounding
    got = runs[0][0][..., :n_off].double().cpu().reshape(B * nq, n_off)
    # element-wise: 50 M sampling points in fp32 against float64 — a handful sit within rounding of a pixel boundary, where floor()
    # (hence the one-sided derivative) legitimately differs; everything else is within one bf16 rounding
    err = (got - want).abs()
    scale = want.abs().max().item()
    outliers = (err > 1e-2 * scale).double().mean().item()
    cos_raw = torch.nn.functional.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    print(f'\n[d offsets, 2 x 98560 x 512] beyond 1e-2 of the scale: {outliers:.2e} of the elements; cosine {cos_raw:.6f}')
    assert outliers <= 1e-4 and cos_raw >= 0.9995, (outliers, cos_raw)
    dW_got, dW_want = got.t() @ query.double(), want.t() @ query.double()      # (512, 64): the weight gradient of the projection
    cos = torch.nn.functional.cosine_similarity(dW_got.flatten(), dW_want.flatten(), dim=0).item()
    ratio = (dW_got.norm() / dW_want.norm()).item()
    print(f'\n[cross-attention offsets projection, 2 x 98560 tokens] weight-gradient cosine {cos:.5f}, norm ratio {ratio:.4f}, d_value run-to-run {dv_noise:.1e}')
    assert cos >= 0.995 and abs(ratio - 1) <= 2e-2, (cos, ratio)


def test_msda_mm_matches_gather_kernels_on_exact_pixel_samples(dev):
    """At initialisation the self-attention samples EXACT pixel positions (pixel-centre reference points + integer offsets), i.e.
    every sample sits on the kink of the bilinear gradient.  The MFMA path computes the locations in mmcv's arithmetic to the bit
    (tools/ubench/msda_mm/divcheck.c: its reciprocal + FMA division is IEEE division for every bf16 offset), so it takes the same one-sided
    derivatives as the gather kernels (ge_msda_fwd_raw / ge_msda_bwd_raw), whose kink decisions the fp32 parity tests pin."""
    from gedepth_amd import kernels as K
    from gedepth_amd.mmrt.bricks import msda_offset_bias
    shapes = [(22, 35), (11, 18), (6, 9), (3, 5)]
    B, nH, L, P = 2, 8, 4, 8
    nq = sum(h * w for h, w in shapes)
    g = gen(29)
    value = torch.randn(B, nq, nH, 64, generator=g).bfloat16().to(dev)
    raw = torch.cat((msda_offset_bias(nH, L, P)[None, None].expand(B, nq, -1), 0.3 * torch.randn(B, nq, nH * L * P, generator=g)), -1).bfloat16().to(dev)
    refs = []
    for h, w in shapes:
        gy, gx = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        refs.append(torch.stack((gx.reshape(-1), gy.reshape(-1)), -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(B, nq, L, 2).contiguous().to(dev)
    go = torch.randn(B, nq, nH * 64, generator=g).bfloat16().to(dev)
    res = []
    for fn in (lambda v, r: K.ms_deform_attn_mm(v, r, ref, shapes, K.msda_tile_order(shapes, dev), nH, L, P),
               lambda v, r: K.ms_deform_attn_raw(v, r, ref, shapes, shapes, nH, L, P)):
        v, r = value.clone().requires_grad_(True), raw.clone().requires_grad_(True)
        out = fn(v, r)
        out.backward(go)
        res.append([t.float().cpu() for t in (out, v.grad, r.grad)])
    for a, b, n in zip(res[0], res[1], ('out', 'd value', 'd raw')):
        close_scaled(a, b, rel=1e-2, what=f'MFMA path vs gather kernels on exact-pixel samples: {n}')


def test_msda_module_golden(dev, golden):
    """Whole MultiScaleDeformableAttention module vs the fixture (mmcv 1.3.13 semantics, dropout off)."""
    from gedepth_amd.depth.models.necks.hahi import MultiScaleDeformableAttention
    g = golden('msda_module')
    spec = json.loads(str(g['spec']))
    m = MultiScaleDeformableAttention(embed_dims=512, num_levels=4, num_heads=8, num_points=8, batch_first=True)
    m.load_state_dict(fill_state_dict([(n, s) for n, s in spec], 'msda_module'))
    m = m.to(dev).eval()
    shapes = [tuple(int(v) for v in s) for s in g['shapes']]
    out = m(T(g['q']).to(dev), value=T(g['v']).to(dev), query_pos=T(g['qp']).to(dev),
            reference_points=T(g['ref']).to(dev), spatial_shapes=shapes)
    close(out, g['out'], rtol=2e-4, atol=2e-5, what='module')


# ============================================================================== bilinear
@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('sizes', [((11, 35), (22, 70)), ((22, 70), (11, 35)), ((7, 9), (16, 31)), ((16, 31), (7, 9)),
                                   ((5, 6), (5, 6)), ((1, 2), (8, 12)), ((176, 560), (352, 1120)), ((11, 35), (176, 560)),
                                   ((3, 5), (13, 17))])
def test_bilinear_fwd_bwd(dev, align, sizes):
    from gedepth_amd.kernels import bilinear_resize
    (hi, wi), (ho, wo) = sizes
    x = torch.randn(2, 3, hi, wi, generator=gen(hi + wo))
    go = torch.randn(2, 3, ho, wo, generator=gen(5))
    xc = x.clone().requires_grad_(True)
    ref = F.interpolate(xc, size=(ho, wo), mode='bilinear', align_corners=align)
    ref.backward(go)
    xg = x.to(dev).requires_grad_(True)
    out = bilinear_resize(xg, (ho, wo), align)
    if out is xg:
        return
    out.backward(go.to(dev))
    close(out, ref, rtol=1e-5, atol=1e-6, what='fwd')
    close(xg.grad, xc.grad, rtol=1e-4, atol=1e-5, what='bwd (deterministic gather)')


def test_bilinear_bwd_is_deterministic_and_adjoint(dev):
    """<up(x), g> == <x, up^T(g)> and bit-identical across runs (no atomics)."""
    from gedepth_amd.kernels import bilinear_resize
    x = torch.randn(4, 8, 88, 280, device=dev, requires_grad=True)
    g = torch.randn(4, 8, 176, 560, device=dev)
    y = bilinear_resize(x, (176, 560), True)
    y.backward(g)
    g1 = x.grad.clone()
    x.grad = None
    bilinear_resize(x, (176, 560), True).backward(g)
    assert torch.equal(g1, x.grad)
    lhs, rhs = (y.detach().double() * g.double()).sum(), (x.detach().double() * g1.double()).sum()
    # fp32 rounding of the 6.3 M products: compare against the Cauchy-Schwarz scale, not against the (random-sign) sum itself
    assert abs(lhs - rhs) <= 1e-6 * y.detach().double().norm() * g.double().norm()


# ====================================================================== ground embedding
def _ground_inputs(B, H, W, seed):
    g = gen(seed)
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = torch.zeros(B, 5, H, W)
    img[:, :3] = torch.randn(B, 3, H, W, generator=g)
    v = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W) * (352.0 / H)
    pe = 1.65 * 721.5377 / (v - 172.854) + 0.05 * torch.randn(B, H, W, generator=g)
    img[:, 4] = pe
    img[:, 3] = torch.where((pe > 0) & (pe <= 200), pe, torch.zeros_like(pe)) / 200.0
    logits = 2.0 * torch.randn(B, 11, h, w, generator=g)
    y = torch.rand(B, 1, h, w, generator=g)
    return img, logits, y


def _oracle_adaptive(img, logits_lr, y_lr, height):
    y = F.interpolate(y_lr, size=img.shape[2:], mode='bilinear')
    pe_mask, logits_hr, m = O.dynamic_pe(logits_lr, y, img[:, 4], 1.65 if height is None else height)
    off_den = None
    return pe_mask, logits_hr, y, m


@pytest.mark.parametrize('hw', [(24, 40), (33, 47), (352, 1120)])
@pytest.mark.parametrize('use_height', [False, True])
def test_ground_embed_adaptive(dev, hw, use_height):
    from gedepth_amd.kernels import ground_embed_adaptive
    B = 2
    img, logits, y = _ground_inputs(B, *hw, seed=hw[0])
    height = torch.tensor([1.56, 1.53]) if use_height else None
    lc, yc = logits.clone().requires_grad_(True), y.clone().requires_grad_(True)
    pe_ref, lg_ref, y_ref, m_ref = _oracle_adaptive(img, lc, yc, height)
    g = gen(3)
    g_pe, g_lg, g_y = (torch.randn(t.shape, generator=g) for t in (pe_ref, lg_ref, y_ref))
    # pixels whose validity is numerically ambiguous (offset within 1e-4 rel of the 200 m threshold or ~0)
    with torch.no_grad():
        hh = 1.65 if height is None else height.view(-1, 1, 1, 1)
        k = torch.tan(torch.deg2rad((F.softmax(lg_ref, 1) * torch.linspace(-5, 5, 11).view(1, 11, 1, 1)).sum(1, keepdim=True)))
        off = -hh / ((-hh / (img[:, 4:5] + 1e-8) - k) + 1e-8)
        ambiguous = ((off - 200.0).abs() < 2e-2) | (off.abs() < 1e-6) | ~torch.isfinite(off)
    (pe_ref * g_pe).sum().backward(retain_graph=True)
    (lg_ref * g_lg).sum().backward(retain_graph=True)
    (y_ref * g_y).sum().backward()

    lg_, yg_ = logits.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    pe, lg_hr, y_hr, valid = ground_embed_adaptive(lg_, yg_, img.to(dev), None if height is None else height.to(dev), 200.0)
    ((pe * g_pe.to(dev)).sum() + (lg_hr * g_lg.to(dev)).sum() + (y_hr * g_y.to(dev)).sum()).backward()

    # integer pixel mask: BIT-EXACT outside the numerically ambiguous set, which must be (almost) empty
    mism = (valid.cpu().bool() != (m_ref[:, 0] == 1)) & ~ambiguous[:, 0]
    assert int(mism.sum()) == 0, f'{int(mism.sum())} mask pixels differ'
    assert int(ambiguous.sum()) <= max(4, ambiguous.numel() // 50000), int(ambiguous.sum())
    assert valid.dtype == torch.uint8 and set(valid.unique().tolist()) <= {0, 1}
    close(lg_hr, lg_ref, rtol=1e-5, atol=5e-6, what='logits_hr')       # a few ulp: ATen's CPU kernel uses fused multiply-adds
    close(y_hr, y_ref, rtol=1e-5, atol=5e-6, what='y_hr')
    ok = ~ambiguous
    close(pe.cpu()[ok], pe_ref[ok], atol=1e-4, what='pe_mask')
    close_scaled(lg_.grad, lc.grad, rel=5e-4, what='d logits_lr')
    close_scaled(yg_.grad, yc.grad, rel=1e-4, what='d y_lr')


def test_ground_embed_integer_mask_vs_reference(dev, golden):
    """north_star: "ground-depth integer pixel mask bit-exact".  ge_ground_embed_fwd's uint8 validity mask against the
    mask read off the reference's own dynamic_pe (tests/golden/make_golden_mask.py) — torch.equal over ALL pixels, no
    excluded set — for 2x24x40 and 2x88x280, default height and per-sample (DDAD) heights."""
    from gedepth_amd.kernels import ground_embed_adaptive
    g = golden('dynamic_pe_mask')
    for tag in 'ab':
        pe_raw = T(g[f'{tag}_pe_raw'])
        B, H, W = pe_raw.shape
        img = torch.zeros(B, 5, H, W)
        img[:, 4] = pe_raw
        img = img.to(dev)
        lg = T(g[f'{tag}_logits_lr']).to(dev)
        ones = torch.ones(B, 1, H // 2, W // 2, device=dev)
        for sfx, h in (('', None), ('_h', T(g[f'{tag}_heights']).to(dev))):
            pe, _, _, valid = ground_embed_adaptive(lg, ones, img, h, 200.0)
            ref = T(g[f'{tag}_mask{sfx}'])[:, 0]
            nd = int((valid.cpu() != ref).sum())
            assert valid.dtype == torch.uint8 and torch.equal(valid.cpu(), ref), f'{tag}{sfx}: {nd} of {ref.numel()} mask pixels differ'
            close(pe.cpu(), g[f'{tag}_offset_masked{sfx}'], rtol=1e-5, atol=1e-4, what='offset * mask')


def test_ground_embed_integer_mask_full_size_vs_oracle(dev):
    """The same all-pixel equality at BASELINE.json's 352x1120 (2 images, 788 k pixels) against the CPU oracle, whose
    mask is itself pinned bit-for-bit to the reference (tests/test_oracle_golden.py)."""
    from gedepth_amd.kernels import ground_embed_adaptive
    for seed, height in ((352, None), (7, torch.tensor([1.56, 1.53]))):
        img, logits, y = _ground_inputs(2, 352, 1120, seed=seed)
        with torch.no_grad():
            _, _, _, m_ref = _oracle_adaptive(img, logits, y, height)
        _, _, _, valid = ground_embed_adaptive(logits.to(dev), y.to(dev), img.to(dev), None if height is None else height.to(dev), 200.0)
        nd = int((valid.cpu() != m_ref[:, 0].to(torch.uint8)).sum())
        assert nd == 0, f'{nd} of {valid.numel()} mask pixels differ from the oracle (seed {seed})'


def test_ground_embed_golden(dev, golden):
    """Against DepthEncoderDecoder.dynamic_pe of the reference itself."""
    from gedepth_amd.kernels import ground_embed_adaptive, ground_embed_vanilla
    g = golden('dynamic_pe')
    img = T(g['img']).to(dev)
    # the fixture's y is given at image resolution; the kernel up-samples a low-res y itself, so run it with
    # y_lr == 1 (=> y_hr == 1) and compare against pe_mask / y of the reference
    y = T(g['y'])
    ones = torch.ones(2, 1, 12, 20, device=dev)
    pe, lg_hr, y_hr, valid = ground_embed_adaptive(T(g['logits_lr']).to(dev), ones, img, None, 200.0)
    assert torch.equal(y_hr, torch.ones_like(y_hr))
    close(lg_hr, g['logits_hr'], rtol=1e-5, atol=1e-6, what='logits')
    close(pe.cpu() * y, g['pe_mask'], atol=1e-4, what='pe_mask')
    pe_h, _, _, _ = ground_embed_adaptive(T(g['logits_lr']).to(dev), ones, img, T(g['heights']).to(dev), 200.0)
    close(pe_h.cpu() * y, g['pe_mask_h'], atol=1e-4, what='pe_mask (per-sample heights)')
    ones_hr = torch.ones(2, 1, 24, 40, device=dev)
    pv, _ = ground_embed_vanilla(ones_hr, img, 200.0)
    close(pv.cpu() * y, g['vanilla'], what='vanilla')


def test_ground_embed_vanilla_bwd(dev):
    from gedepth_amd.kernels import ground_embed_vanilla
    img, _, y = _ground_inputs(2, 30, 52, seed=8)
    yc = y.clone().requires_grad_(True)
    yu = F.interpolate(yc, size=img.shape[2:], mode='bilinear')
    ref = O.vanilla_pe(yu, img[:, 3])
    g = gen(1)
    g1, g2 = torch.randn(ref.shape, generator=g), torch.randn(ref.shape, generator=g)
    ((ref * g1).sum() + (yu * g2).sum()).backward()
    yg = y.to(dev).requires_grad_(True)
    pe, yh = ground_embed_vanilla(yg, img.to(dev), 200.0)
    ((pe * g1.to(dev)).sum() + (yh * g2.to(dev)).sum()).backward()
    close(pe, ref, what='pe_mask')
    close_scaled(yg.grad, yc.grad, what='d y_lr')


def test_depth_fuse(dev):
    from gedepth_amd.kernels import depth_fuse
    B, h, w, H, W = 2, 20, 31, 40, 62
    g = gen(2)
    c = torch.randn(B, 1, h, w, generator=g)
    pe = torch.rand(B, 1, H, W, generator=g) * 50
    y = torch.rand(B, 1, H, W, generator=g)
    go = torch.randn(B, 1, h, w, generator=g)
    cc, pc, yc = (t.clone().requires_grad_(True) for t in (c, pe, y))
    d = F.relu(cc)
    ref = (d * (1 - F.interpolate(yc, size=(h, w), mode='bilinear', align_corners=True))
           + F.interpolate(pc, size=(h, w), mode='bilinear', align_corners=True)) + 1e-3
    ref.backward(go)
    cg, pg, yg = (t.to(dev).requires_grad_(True) for t in (c, pe, y))
    out, _ = depth_fuse(cg, pg, yg, 1e-3)
    out.backward(go.to(dev))
    close(out, ref, what='out')
    close_scaled(cg.grad, cc.grad, what='d conv')
    close_scaled(pg.grad, pc.grad, what='d pe_mask')
    close_scaled(yg.grad, yc.grad, what='d y')

@pytest.mark.gpu
@pytest.mark.parametrize('P', [8, 4])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_msda_prepare_matches_mmcv_arithmetic(dev, P, dtype):
    """view -> softmax over L*P -> reference_points + offsets / (W_l, H_l) of mmcv MultiScaleDeformableAttention.forward,
    forward and backward (incl. the gradient of broadcast reference points), against the ATen sequence."""
    from gedepth_amd.kernels import msda_prepare
    B, Nq, nH, L = 2, 37, 8, 4
    shapes = [(12, 20), (6, 10), (3, 5), (2, 3)]
    g = gen(11)
    n_off, n_log = nH * L * P * 2, nH * L * P
    raw = torch.randn(B, Nq, n_off + n_log, generator=g) * 2
    ref0 = torch.rand(1, Nq, 2, generator=g)
    g_loc = torch.randn(B, Nq, nH, L, P, 2, generator=g)
    g_w = torch.randn(B, Nq, nH, L, P, generator=g)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    raw = raw.to(td).float()                                                # same stored values on both sides
    rc, fc = raw.clone().requires_grad_(True), ref0.clone().requires_grad_(True)
    off = rc[..., :n_off].view(B, Nq, nH, L, P, 2)
    w_ref = rc[..., n_off:].view(B, Nq, nH, L * P).softmax(-1).view(B, Nq, nH, L, P)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)
    loc_ref = fc[:, :, None, :].expand(B, -1, L, 2)[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    (loc_ref * g_loc).sum().add((w_ref * g_w).sum()).backward()
    rg = raw.to(dev).to(td).requires_grad_(True)
    fg = ref0.to(dev).requires_grad_(True)
    loc, w = msda_prepare(rg, fg[:, :, None, :].expand(B, -1, L, 2), shapes, nH, L, P)
    (loc * g_loc.to(dev)).sum().add((w * g_w.to(dev)).sum()).backward()
    close(loc, loc_ref, what='loc')
    close(w, w_ref, what='attw')
    if dtype == 'f32':
        close_scaled(rg.grad, rc.grad, what='d raw')
    else:
        assert (rg.grad.float().cpu() - rc.grad).abs().max() <= 2 ** -8 * rc.grad.abs().max() + 1e-6
    close_scaled(fg.grad, fc.grad, what='d reference points')


@pytest.mark.gpu
@pytest.mark.parametrize('geom', [(2, 16, 4, 6), (2, 64, 8, 16), (1, 7, 3, 5), (3, 72, 9, 8)])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_tokens_from_map_and_back(dev, geom, dtype):
    """flatten(2).transpose(1,2) + pos (hahi.py:303-306) and its inverse with residual + concat (hahi.py:326-333)."""
    from gedepth_amd.kernels import concat_tokens_map, tokens_from_map
    B, C, H, W = geom
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = gen(3)
    fmap = torch.randn(B, C, H, W, generator=g).to(td)
    pos = torch.randn(1, C, H, W, generator=g)
    other = torch.randn(B, 5, H, W, generator=g).to(td)
    go = torch.randn(B, C + 5, H, W, generator=g).to(td)
    for first in (True, False):
        fc, oc = fmap.float().clone().requires_grad_(True), other.float().clone().requires_grad_(True)
        tok_ref = fc.flatten(2).transpose(1, 2) + pos.flatten(2).transpose(1, 2)
        tok_ref_q = tok_ref.to(td).float()
        proc = tok_ref * 0.5                                            # stand-in for the attention block
        m = proc.permute(0, 2, 1).reshape(B, C, H, W) + fc
        ref = torch.cat([m, oc] if first else [oc, m], 1)
        ref.backward(go.float())
        fg, og = fmap.to(dev).requires_grad_(True), other.to(dev).requires_grad_(True)
        tok = tokens_from_map(fg, pos.to(dev))
        assert tok.shape == (B, H * W, C) and tok.is_contiguous()
        out = concat_tokens_map(tok * 0.5, og, identity=fg, tokens_first=first)
        out.backward(go.to(dev))
        tol = dict(rtol=2 ** -7, atol=2 ** -7) if dtype == 'bf16' else {}
        close(tok.float(), tok_ref_q if dtype == 'bf16' else tok_ref, what='tokens', **tol)
        close(out.float(), ref, what='concat', **tol)
        close(fg.grad.float(), fc.grad, what='d map', **tol)
        close(og.grad.float(), oc.grad, what='d other', **tol)


@pytest.mark.gpu
def test_concat_tokens_map_token_slice_and_dropout(dev):
    """Token ranges of a longer sequence (hahi.py:338-346) and the counter-based dropout: keep rate, 1/(1-p) scaling,
    identical mask in forward and backward, reproducible for a seed."""
    from gedepth_amd.kernels import concat_tokens_map
    B, C, H, W = 2, 64, 16, 24
    g = gen(4)
    seq = torch.randn(B, 3 * H * W, C, generator=g).to(dev)
    ft = torch.randn(B, 8, H, W, generator=g).to(dev)
    sl = seq[:, H * W:2 * H * W]
    out = concat_tokens_map(sl, ft, tokens_first=False)
    assert torch.equal(out[:, 8:], sl.permute(0, 2, 1).reshape(B, C, H, W)) and torch.equal(out[:, :8], ft)
    p = 0.25
    tok = torch.ones(B, H * W, C, device=dev, requires_grad=True)
    o1 = concat_tokens_map(tok, ft, tokens_first=True, p_drop=p, seed=1234)
    o2 = concat_tokens_map(tok, ft, tokens_first=True, p_drop=p, seed=1234)
    o3 = concat_tokens_map(tok, ft, tokens_first=True, p_drop=p, seed=1235)
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)
    kept = o1[:, :C] != 0
    assert abs(kept.float().mean().item() - (1 - p)) < 0.01
    assert torch.allclose(o1[:, :C][kept], torch.full((), 1 / (1 - p), device=dev))
    assert abs(kept.float().mean((0, 2, 3)).min().item() - (1 - p)) < 0.06        # no dead channel / striping
    o1[:, :C].sum().backward()
    assert torch.equal(tok.grad != 0, kept.flatten(2).transpose(1, 2))
    assert torch.allclose(tok.grad[tok.grad != 0], torch.full((), 1 / (1 - p), device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize('C', [96, 192, 384, 768, 1536, 3072, 100])
@pytest.mark.parametrize('io', ['f32->f32', 'f32->bf16', 'bf16->bf16', 'bf16->f32'])
def test_layer_norm_mixed_precision(dev, C, io):
    """F.layer_norm on the Swin token path (norm1 / norm2 / PatchMerging.norm / stage norms) with the dtype copies autocast
    puts around it folded in; forward and all three gradients against the fp32 ATen op on the same stored values."""
    from gedepth_amd.kernels import layer_norm
    tin, tout = (torch.float32 if t == 'f32' else torch.bfloat16 for t in io.split('->'))
    rows = (3, 37)
    g = gen(21)
    x = (torch.randn(*rows, C, generator=g) * 2 + 0.5).to(tin)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    go = torch.randn(*rows, C, generator=g).to(tout)
    xc, wc, bc = x.float().clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xc, (C,), wc, bc, 1e-5)
    ref.backward(go.float())
    xg, wg, bg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = layer_norm(xg, wg, bg, 1e-5, tout)
    assert out.dtype == tout and xg.shape == out.shape
    out.backward(go.to(dev))
    assert xg.grad.dtype == tin
    t_out = dict(rtol=2 ** -7, atol=2 ** -7) if tout == torch.bfloat16 else dict(rtol=1e-5, atol=1e-5)
    close(out.float(), ref, what='y', **t_out)
    if tin == torch.bfloat16:
        assert (xg.grad.float().cpu() - xc.grad).abs().max() <= 2 ** -7 * xc.grad.abs().max()
    else:
        close_scaled(xg.grad, xc.grad, what='dx')
    close_scaled(wg.grad, wc.grad, what='dgamma')
    close_scaled(bg.grad, bc.grad, what='dbeta')


@pytest.mark.gpu
def test_layer_norm_module_follows_autocast(dev):
    from gedepth_amd.mmrt.bricks import build_norm_layer
    ln = build_norm_layer(dict(type='LN'), 96)[1].to(dev)
    x = torch.randn(2, 50, 96, device=dev)
    assert ln(x).dtype == torch.float32
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert ln(x).dtype == torch.bfloat16 and ln(x.bfloat16()).dtype == torch.bfloat16
        ln.autocast_out = False
        assert ln(x.bfloat16()).dtype == torch.float32
    assert torch.allclose(ln(x), F.layer_norm(x, (96,), ln.weight, ln.bias, ln.eps), atol=1e-5, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('autocast', [False, True])
def test_linear_tokens_split_k_weight_gradient(dev, autocast):
    """Linear over a large token matrix: output and all gradients equal F.linear's (the weight gradient is summed over
    token chunks in fp32 instead of one library GEMM)."""
    from gedepth_amd.mmrt.bricks import Linear, _split_k
    assert _split_k(788480) == 64 and _split_k(261800) == 56 and _split_k(49280) == 44 and _split_k(4000) == 0
    torch.manual_seed(0)
    lin = Linear(96, 160).to(dev)
    x = torch.randn(2, 24640, 96, device=dev, requires_grad=True)          # 49280 tokens -> 44 chunks
    go = torch.randn(2, 24640, 160, device=dev)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        y = lin(x)
        ref = F.linear(x, lin.weight, lin.bias)
    assert y.dtype == ref.dtype and torch.equal(y, ref)
    y.backward(go.to(y.dtype))
    gx, gw, gb = x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()
    x.grad = None; lin.zero_grad()
    ref.backward(go.to(ref.dtype))
    tol = 2e-2 if autocast else 1e-4                                        # bf16: the library rounds dW to bf16, split-K does not
    assert (gx - x.grad).norm() <= tol * x.grad.norm()
    assert (gw - lin.weight.grad).norm() <= tol * lin.weight.grad.norm()
    assert (gb - lin.bias.grad).norm() <= tol * lin.bias.grad.norm()
    if autocast:                                                            # and it is the more accurate of the two
        exact = go.reshape(-1, 160).bfloat16().double().t() @ x.detach().reshape(-1, 96).bfloat16().double()
        assert (gw.double() - exact).norm() <= (lin.weight.grad.double() - exact).norm()


@pytest.mark.gpu
@pytest.mark.parametrize('dtypes', ['f32+f32', 'f32+bf16', 'bf16+bf16'])
@pytest.mark.parametrize('shape', [(4, 37, 96), (3, 5, 7)])
def test_residual_drop_path(dev, dtypes, shape):
    """identity + DropPath(branch) of the Swin blocks: mixed-precision single pass and its backward vs ATen, and the
    DropPath module draws the same per-sample mask as the unfused formula."""
    from gedepth_amd.kernels import residual_drop_path
    from gedepth_amd.mmrt.bricks import DropPath, drop_path
    ti, tb = (torch.float32 if t == 'f32' else torch.bfloat16 for t in dtypes.split('+'))
    g = gen(8)
    ident, br = torch.randn(*shape, generator=g).to(ti), torch.randn(*shape, generator=g).to(tb)
    scale = torch.tensor([0.0, 1 / 0.7, 1 / 0.7, 0.0][:shape[0]])
    go = torch.randn(*shape, generator=g).to(ti)
    ic, bc = ident.float().clone().requires_grad_(True), br.float().clone().requires_grad_(True)
    ref = ic + bc * scale.view(-1, 1, 1)
    ref.backward(go.float())
    ig, bg = ident.to(dev).requires_grad_(True), br.to(dev).requires_grad_(True)
    out = residual_drop_path(ig, bg, scale.to(dev))
    assert out.dtype == ti
    out.backward(go.to(dev))
    tol = dict(rtol=2 ** -7, atol=2 ** -7) if ti == torch.bfloat16 else dict(rtol=1e-6, atol=1e-6)
    close(out.float(), ref, what='out', **tol)
    close(ig.grad.float(), ic.grad, what='d identity', **tol)
    assert bg.grad.dtype == tb
    close(bg.grad.float(), bc.grad, what='d branch', **(dict(rtol=2 ** -7, atol=2 ** -7) if tb == torch.bfloat16 else tol))
    # the module: scales come from the shared bank (one uniform draw per step for all DropPath layers, bricks._DropPathBank): every
    # sample is either dropped (identity) or kept (identity + branch / keep), and the keep rate follows 1 - p
    m, m2 = DropPath(0.3).to(dev).train(), DropPath(0.6).to(dev).train()
    kept = [0, 0]
    for it in range(40):
        for k, (mod, keep) in enumerate(((m, 0.7), (m2, 0.4))):
            fused = mod.residual(ident.to(dev), br.to(dev)).float().cpu()
            lo, hi = ident.float(), ident.float() + br.float() / keep
            for b_ in range(shape[0]):
                is_lo = torch.allclose(fused[b_], lo[b_].to(ti).float(), rtol=2 ** -7, atol=2 ** -7)
                is_hi = torch.allclose(fused[b_], hi[b_], rtol=2 ** -6, atol=2 ** -6)
                assert is_lo or is_hi, 'a sample is neither dropped nor kept'
                kept[k] += int(is_hi and not is_lo)
    n = 40 * shape[0]
    assert abs(kept[0] / n - 0.7) < 0.15 and abs(kept[1] / n - 0.4) < 0.15, kept
    assert drop_path(br, 0.0, True) is br


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 5, 7, 9), (3, 16, 12, 16), (2, 64, 24, 40)])
@pytest.mark.parametrize('slope', [0.0, 1.0])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bn_act_training(dev, shape, slope, dtype):
    """nn.BatchNorm2d (training) + ReLU of mmcv ConvModule: output, running statistics, num_batches_tracked and the three
    gradients against F.batch_norm + relu in fp32 on the same stored values."""
    from gedepth_amd.kernels import bn_act
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = gen(31)
    N, C, H, W = shape
    x = (torch.randn(*shape, generator=g) * 1.5 + 0.3).to(td)
    go = torch.randn(*shape, generator=g).to(td)
    ref_bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        ref_bn.weight.copy_(torch.randn(C, generator=g)); ref_bn.bias.copy_(torch.randn(C, generator=g))
        ref_bn.running_mean.copy_(torch.randn(C, generator=g)); ref_bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    import copy
    bn = copy.deepcopy(ref_bn).to(dev)
    xc = x.float().clone().requires_grad_(True)
    t = ref_bn(xc)
    ref = t if slope == 1.0 else F.relu(t)
    ref.backward(go.float())
    xg = x.to(dev).requires_grad_(True)
    out = bn_act(xg, bn, slope)
    out.backward(go.to(dev))
    tol = dict(rtol=2 ** -7, atol=2 ** -7) if dtype == 'bf16' else dict(rtol=2e-5, atol=2e-5)
    close(out.float(), ref, what='y', **tol)
    close(bn.running_mean, ref_bn.running_mean, rtol=1e-5, atol=1e-6, what='running_mean')
    close(bn.running_var, ref_bn.running_var, rtol=1e-5, atol=1e-6, what='running_var')
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1
    if dtype == 'bf16':
        # a bf16-rounded y flips relu'(y) only where |y| is at rounding level: compare in norm
        assert (xg.grad.float().cpu() - xc.grad).norm() <= 2e-2 * xc.grad.norm()
        assert (bn.weight.grad.cpu() - ref_bn.weight.grad).norm() <= 2e-2 * ref_bn.weight.grad.norm()
        assert (bn.bias.grad.cpu() - ref_bn.bias.grad).norm() <= 2e-2 * ref_bn.bias.grad.norm()
    else:
        close_scaled(xg.grad, xc.grad, what='dx')
        close_scaled(bn.weight.grad, ref_bn.weight.grad, what='dgamma')
        close_scaled(bn.bias.grad, ref_bn.bias.grad, what='dbeta')


@pytest.mark.parametrize('shape,cout,mode', [((2, 64, 24, 40), 512, 'both'), ((3, 64, 7, 9), 256, 'both'), ((2, 64, 16, 20), 128, 'map'),
                                             ((1, 64, 33, 17), 512, 'tokens'), ((2, 64, 24, 40), 512, 'slice')])
def test_conv1x1_bn_act_pos_vs_fp32_composition(dev, shape, cout, mode):
    """csrc/conv1x1_bn.hip: ConvModule(64 -> Cout, 1x1, BN, ReLU) + the query's position add (reference necks/hahi.py:151-157,294-306) in one pass,
    BatchNorm statistics from the input's Gram matrix — against conv2d -> batch_norm(training) -> relu -> + pos in fp32 on the same bf16 inputs
    and bf16-rounded weights: both outputs, running statistics, and all four gradients (the BatchNorm backward is rank-64 algebra there, see the
    file header).  ``slice``: the gradient of the map arrives as a channel slice of a wider channels-last map (torch.cat backward) and is read
    in place; ``map`` / ``tokens``: only one of the two outputs is used."""
    from gedepth_amd import kernels as K
    from gedepth_amd.mmrt.bricks import ConvModule
    g = gen(77)
    B, Cin, H, W = shape
    block = ConvModule(Cin, cout, 1, norm_cfg=dict(type='BN', requires_grad=True), act_cfg=dict(type='ReLU'))
    with torch.no_grad():
        block.conv.weight.copy_(torch.randn(cout, Cin, 1, 1, generator=g) * 0.2)
        block.bn.weight.copy_(torch.rand(cout, generator=g) + 0.5); block.bn.bias.copy_(torch.randn(cout, generator=g) * 0.3)
        block.bn.running_mean.copy_(torch.randn(cout, generator=g)); block.bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    import copy
    ref = copy.deepcopy(block)
    block = block.to(dev).train()
    x = (torch.relu(torch.randn(*shape, generator=g)) * 1.3 + 0.1).to(torch.bfloat16)            # post-ReLU statistics: mean comparable to the deviation
    pos = torch.randn(1, cout, H, W, generator=g)
    gy = torch.randn(B, cout, H, W, generator=g).to(torch.bfloat16)
    gq = torch.randn(B, H * W, cout, generator=g).to(torch.bfloat16)
    extra = torch.randn(B, 32, H, W, generator=g).to(torch.bfloat16)
    # ---- fp32 composition on the CPU
    xr = x.float().clone().requires_grad_(True)
    wr = ref.conv.weight.detach().to(torch.bfloat16).float().requires_grad_(True)
    z = F.conv2d(xr, wr)
    yr = F.relu(F.batch_norm(z, ref.bn.running_mean, ref.bn.running_var, ref.bn.weight, ref.bn.bias, True, ref.bn.momentum, ref.bn.eps))
    qr = yr.flatten(2).transpose(1, 2) + pos.flatten(2).transpose(1, 2)
    loss = 0
    if mode != 'tokens':
        loss = loss + (yr * gy.float()).sum()
    if mode != 'map':
        loss = loss + (qr * gq.float()).sum()
    loss.backward()
    # ---- the fused kernels
    xg = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert K.conv1x1_bn_act_pos_ok(block, xg)
        y, q = K.conv1x1_bn_act_pos(block, xg, pos.to(dev))
    assert y.dtype == q.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    out = 0
    if mode == 'slice':
        wide = torch.cat([y, extra.to(dev).contiguous(memory_format=torch.channels_last)], 1)
        out = out + (wide.float() * torch.cat([gy, torch.zeros_like(extra)], 1).to(dev).float()).sum()
    elif mode != 'tokens':
        out = out + (y.float() * gy.to(dev).float()).sum()
    if mode != 'map':
        out = out + (q.float() * gq.to(dev).float()).sum()
    out.backward()
    close(y.float(), yr, rtol=2 ** -7, atol=2 ** -7, what='y')
    close(q.float(), qr, rtol=2 ** -7, atol=2 ** -6, what='q')
    close(block.bn.running_mean, ref.bn.running_mean, rtol=1e-4, atol=1e-5, what='running_mean')
    close(block.bn.running_var, ref.bn.running_var, rtol=1e-4, atol=1e-5, what='running_var')
    assert int(block.bn.num_batches_tracked) == 1
    # gradients: the masked gradient g is stored in bf16 (as the two-pass path stores dy), relu'(y) flips where |y| is at rounding level
    errs = dict(dx=l2rel(xg.grad.float(), xr.grad), dw=l2rel(block.conv.weight.grad, wr.grad), dgamma=l2rel(block.bn.weight.grad, ref.bn.weight.grad),
                dbeta=l2rel(block.bn.bias.grad, ref.bn.bias.grad))
    print(f'\n[conv1x1_bn {shape}->{cout} {mode}] l2 errors', {k: f'{v:.2e}' for k, v in errs.items()})
    assert errs['dx'] <= 1e-2 and errs['dw'] <= 6e-3 and errs['dgamma'] <= 6e-3 and errs['dbeta'] <= 6e-3, errs


@pytest.mark.parametrize('shape,cout', [((2, 96, 24, 40), 512), ((8, 768, 11, 35), 768), ((2, 64, 88, 140), 64)])            # the last: 24 640 rows, split-K weight gradient
def test_conv1x1_as_token_gemm_vs_fp32_conv(dev, shape, cout):
    """kernels._Conv1x1Gemm: a bias-free 1x1 convolution of a channels-last bf16 map as a token GEMM (forward, data gradient, split-K or plain
    weight gradient in fp32) against F.conv2d in fp32 on the same bf16 inputs and bf16-rounded weight."""
    from gedepth_amd import kernels as K
    g = gen(91)
    B, Cin, H, W = shape
    conv = torch.nn.Conv2d(Cin, cout, 1, bias=False)
    x = torch.randn(*shape, generator=g).to(torch.bfloat16)
    gy = torch.randn(B, cout, H, W, generator=g).to(torch.bfloat16)
    xr = x.float().clone().requires_grad_(True)
    wr = conv.weight.detach().to(torch.bfloat16).float().requires_grad_(True)
    yr = F.conv2d(xr, wr)
    yr.backward(gy.float())
    conv = conv.to(dev)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert K.conv1x1_gemm_ok(conv, xg)
        y = K.conv_lib(conv, xg)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last) and tuple(y.shape) == (B, cout, H, W)
    y.backward(gy.to(dev).contiguous(memory_format=torch.channels_last))
    errs = dict(y=l2rel(y.float(), yr), dx=l2rel(xg.grad.float(), xr.grad), dw=l2rel(conv.weight.grad, wr.grad))
    print(f'\n[conv1x1 as GEMM {shape}->{cout}]', {k: f'{v:.2e}' for k, v in errs.items()})
    assert errs['y'] <= 4e-3 and errs['dx'] <= 4e-3 and errs['dw'] <= 4e-3, errs          # bf16 storage of y / dx; dW: bf16 split-K partials


@pytest.mark.gpu
def test_conv_module_bn_relu_fused_matches_unfused(dev):
    from gedepth_amd.mmrt.bricks import ConvModule
    torch.manual_seed(0)
    m = ConvModule(8, 16, 3, padding=1, norm_cfg=dict(type='BN', requires_grad=True), act_cfg=dict(type='ReLU')).to(dev).train()
    x = torch.randn(2, 8, 24, 40, device=dev)
    go = torch.randn(2, 16, 24, 40, device=dev)
    out = m(x)
    out.backward(go)
    gw, gg = m.conv.weight.grad.clone(), m.bn.weight.grad.clone()
    rm = m.bn.running_mean.clone()
    m.zero_grad(); m.bn.reset_running_stats()
    ref = F.relu(F.batch_norm(F.conv2d(x, m.conv.weight, None, padding=1), m.bn.running_mean, m.bn.running_var, m.bn.weight,
                              m.bn.bias, True, 0.1, 1e-5))
    ref.backward(go)
    close(out, ref, rtol=1e-4, atol=1e-4, what='y')
    close_scaled(gw, m.conv.weight.grad, what='d conv weight')
    close_scaled(gg, m.bn.weight.grad, what='dgamma')
    close(rm, m.bn.running_mean, rtol=1e-5, atol=1e-6, what='running_mean')
    m.eval()
    assert torch.allclose(m(x), F.relu(m.bn(m.conv(x))))                      # eval mode: the library path


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 5, 7, 9), (2, 16, 12, 16), (1, 3, 1, 1)])
@pytest.mark.parametrize('slope', [1.0, 0.0, 0.01])
def test_bias_act_fp32(dev, shape, slope):
    """conv output + bias + (leaky) ReLU in one pass (ConvModule without norm, PE-neck convs) vs ATen."""
    from gedepth_amd.kernels import bias_act_
    g = gen(5)
    x = torch.randn(*shape, generator=g)
    b = torch.randn(shape[1], generator=g)
    go = torch.randn(*shape, generator=g)
    xc, bc = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    t = xc + bc.view(1, -1, 1, 1)
    ref = t if slope == 1.0 else F.leaky_relu(t, slope)
    ref.backward(go)
    xg, bg = x.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = bias_act_(xg * 1.0, bg, slope)          # in place on a non-leaf, like a conv output
    out.backward(go.to(dev))
    close(out, ref, what='out')
    close(xg.grad, xc.grad, what='dx')
    close_scaled(bg.grad, bc.grad, what='dbias')


@pytest.mark.gpu
def test_conv_module_fused_bias_act_bf16(dev):
    """ConvModule(conv+bias+LeakyReLU) through the fused kernel under autocast vs the unfused ATen sequence."""
    from gedepth_amd.mmrt.bricks import ConvModule
    torch.manual_seed(0)
    m = ConvModule(8, 16, 3, padding=1, act_cfg=dict(type='LeakyReLU', negative_slope=0.01)).to(dev)
    x = torch.randn(2, 8, 24, 40, device=dev)
    go = torch.randn(2, 16, 24, 40, device=dev)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = m(x)
    assert out.dtype == torch.bfloat16
    out.float().backward(go)
    gw, gb = m.conv.weight.grad.clone(), m.conv.bias.grad.clone()
    m.zero_grad()
    with torch.autocast('cuda', dtype=torch.bfloat16):          # same bf16 convolution, epilogue by ATen in fp32
        y = F.conv2d(x, m.conv.weight, None, padding=1)
    ref = F.leaky_relu(y.float() + m.conv.bias.view(1, -1, 1, 1), 0.01)
    ref.backward(go)
    assert (out.float() - ref).abs().max() <= 2 ** -8 * ref.abs().max()            # one bf16 rounding of the output
    assert (gb - m.conv.bias.grad).norm() <= 1e-2 * m.conv.bias.grad.norm()         # dy rounded to bf16
    assert (gw - m.conv.weight.grad).norm() <= 1e-2 * m.conv.weight.grad.norm()


def test_silog(dev, golden):
    from gedepth_amd.kernels import silog_loss
    g = golden('known_answers')
    out = silog_loss(T(g['sig_pred']).to(dev).view(1, 1, 2, 4), T(g['sig_gt']).to(dev).view(1, 1, 2, 4))
    assert abs(out.item() - 0.28163391) < 1e-6
    gg = gen(4)
    pred = torch.rand(2, 1, 64, 96, generator=gg) * 80 + 0.1
    gt = torch.where(torch.rand(2, 1, 64, 96, generator=gg) < 0.3, torch.rand(2, 1, 64, 96, generator=gg) * 80, torch.zeros(2, 1, 64, 96))
    pc = pred.clone().requires_grad_(True)
    ref = O.sigloss(pc, gt)
    ref.backward()
    pg = pred.to(dev).requires_grad_(True)
    out = silog_loss(pg, gt.to(dev))
    out.backward()
    close(out, ref, rtol=1e-5, what='loss')
    close_scaled(pg.grad, pc.grad, what='d pred')


# ============================================================== offline ground-plane maps
def test_ground_plane_and_slope_class_bit_exact(dev):
    from gedepth_amd.kernels import ground_plane, pe_channels, slope_class
    P2 = np.array([[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01],
                   [0.0, 0.0, 1.0, 2.745884e-03]])
    Tr = np.array([[0., -1, 0, 0], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]])
    H, W = 375, 1242
    pe_ref, r2, num = O.ground_plane(P2, np.eye(3), Tr, H, W)
    pe64, pe32 = ground_plane(r2, num, H, W, device=dev)
    assert np.array_equal(pe64.cpu().numpy(), pe_ref)                        # float64, bit-exact
    assert np.array_equal(pe32.cpu().numpy(), pe_ref.astype(np.float32))
    np.testing.assert_allclose(pe64[374, 621].item(), 5.630516794, rtol=1e-9)
    rs = np.random.RandomState(0)
    gt = np.where(rs.rand(H, W) < 0.2, np.round(rs.rand(H, W) * 80 * 256) / 256.0, 0.0)
    for mode in ('round', 'trunc'):
        k_ref = O.slope_class(gt, pe_ref.astype(np.float32), 1.65, mode)
        k = slope_class(torch.from_numpy(gt).to(dev), pe32, 1.65, mode).cpu().numpy()
        assert k.dtype == np.int16
        assert np.array_equal(k.astype(np.float64), k_ref), int((k != k_ref).sum())
    norm_ref, raw_ref = O.loader_pe_channels(pe_ref)
    assert np.array_equal(pe_channels(pe32).cpu().numpy(), norm_ref)
    k = slope_class(torch.tensor([[10., 0], [30, 5]], dtype=torch.float64, device=dev),
                    torch.tensor([[11, 20], [25, 5.2]], device=dev))
    assert k.tolist() == [[1, 255], [-1, 1]]


# ================================================================================ AdamW
def test_fused_adamw_matches_torch(dev):
    from gedepth_amd.mmrt.optim import FusedAdamW
    torch.manual_seed(0)
    shapes = [(33, 7), (129,), (5, 3, 3, 3), (1,)]
    ref_params = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes]
    our_params = [p.detach().clone().requires_grad_(True) for p in ref_params]
    ref = torch.optim.AdamW([dict(params=ref_params[:2], weight_decay=0.01), dict(params=ref_params[2:], weight_decay=0.0)],
                            lr=1e-3, betas=(0.9, 0.999))
    ours = FusedAdamW([dict(params=our_params[:2], weight_decay=0.01), dict(params=our_params[2:], weight_decay=0.0)],
                      lr=1e-3, betas=(0.9, 0.999), max_grad_norm=0.5)
    for step in range(5):
        grads = [torch.randn(s, device=dev) for s in shapes]
        for p, q, g in zip(ref_params, our_params, grads):
            p.grad = g.clone()
            q.grad.copy_(g)                 # .grad is a view into the flat gradient arena
        torch.nn.utils.clip_grad_norm_(ref_params, 0.5)
        ref.step()
        ours.step()
        for p, q in zip(ref_params, our_params):
            close(q, p, rtol=1e-5, atol=1e-7, what=f'step {step}')


def test_fused_adamw_state_dict_is_torch_layout(dev):
    """Checkpoint interop (mmcv layout: 'optimizer' = a torch.optim state dict): a torch.optim.AdamW state loads into
    FusedAdamW and vice versa, and training continues identically; mismatching shapes are refused before any copy."""
    from gedepth_amd.mmrt.optim import FusedAdamW
    torch.manual_seed(1)
    shapes = [(17, 5), (40,), (3, 2, 3, 3)]
    mk = lambda: [torch.randn(s, device=dev, generator=torch.Generator(dev).manual_seed(7 + i)).requires_grad_(True)
                  for i, s in enumerate(shapes)]
    groups = lambda ps: [dict(params=[ps[0]], weight_decay=0.01), dict(params=[ps[1]], weight_decay=0.0),
                         dict(params=[ps[2]], weight_decay=0.01)]
    tp, fp = mk(), mk()
    ref = torch.optim.AdamW(groups(tp), lr=2e-3)
    ours = FusedAdamW(groups(fp), lr=2e-3)

    def both(n):
        for _ in range(n):
            grads = [torch.randn(s, device=dev) for s in shapes]
            for p, q, g in zip(tp, fp, grads):
                p.grad = g.clone()
                q.grad.copy_(g)
            ref.step()
            ours.step()
    both(2)
    sd = ours.state_dict()
    assert set(sd) == {'state', 'param_groups'} and set(sd['state']) == {0, 1, 2}
    assert [g['params'] for g in sd['param_groups']] == [[0], [1], [2]]
    assert tuple(sd['state'][2]['exp_avg'].shape) == shapes[2] and float(sd['state'][0]['step']) == 2.0
    for i in range(3):
        close(sd['state'][i]['exp_avg_sq'], ref.state_dict()['state'][i]['exp_avg_sq'], rtol=1e-5, atol=1e-9, what='exp_avg_sq')
    # torch -> fused: a fresh FusedAdamW resumes from the torch optimizer's checkpoint
    fp2 = [p.detach().clone().requires_grad_(True) for p in tp]
    ours2 = FusedAdamW(groups(fp2), lr=2e-3)
    ours2.load_state_dict(ref.state_dict())
    # fused -> torch
    tp2 = [p.detach().clone().requires_grad_(True) for p in fp]
    ref2 = torch.optim.AdamW(groups(tp2), lr=2e-3)
    ref2.load_state_dict(sd)
    grads = [torch.randn(s, device=dev) for s in shapes]
    for plist, opt in ((tp, ref), (fp2, ours2), (tp2, ref2)):
        for p, g in zip(plist, grads):
            if opt is ours2:
                p.grad.copy_(g)
            else:
                p.grad = g.clone()
        opt.step()
    for a, b, c in zip(tp, fp2, tp2):
        close(b, a, rtol=1e-5, atol=1e-7, what='torch state -> FusedAdamW')
        close(c, a, rtol=1e-5, atol=1e-7, what='FusedAdamW state -> torch')
    bad = ref.state_dict()
    bad['state'][1]['exp_avg'] = torch.zeros(41)
    before = ours2.exp_avg.clone()
    with pytest.raises(ValueError):
        ours2.load_state_dict(bad)
    assert torch.equal(before, ours2.exp_avg)                      # nothing was copied
    with pytest.raises(ValueError):
        ours2.load_state_dict(dict(step=1, exp_avg=torch.zeros(5), exp_avg_sq=torch.zeros(5), param_groups=[]))


def test_ground_plane_and_slope_classes_vs_reference_scripts(dev, golden):
    """ge_ground_plane / ge_slope_class / ge_slope_class_ddad bit-for-bit against the arrays the reference's own
    tools/preprocess_data_kitti.py and preprocess_data_ddad.py wrote for a toy calibration tree
    (tests/golden/make_golden_ground.py): float64 maps, integer class maps, every pixel."""
    sys_path_tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    import importlib.util
    from gedepth_amd.kernels import ground_plane, slope_class, slope_class_ddad
    spec = importlib.util.spec_from_file_location('pp_ddad', os.path.join(sys_path_tools, 'preprocess_data_ddad.py'))
    pp_ddad = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pp_ddad)
    g = golden('ground_plane')
    for d in range(2):
        ref = g[f'kitti{d}_pe']
        H, W = ref.shape
        R0, Tr = np.eye(4), g[f'kitti{d}_Tr']
        R0[:3, :3] = g[f'kitti{d}_R0']
        A = g[f'kitti{d}_P2'] @ R0 @ Tr                     # host side of tools/preprocess_data_kitti.py (this repo)
        Rinv = np.linalg.inv(A[:3, :3])
        RT = Rinv @ A[:3, 3]
        pe64, pe32 = ground_plane(Rinv[2], float(RT[2] - 1.65), H, W, device=dev)
        assert np.array_equal(pe64.cpu().numpy(), ref), 'pe float64 map differs from the reference script'
        assert np.array_equal(pe32.cpu().numpy(), ref.astype(np.float32))
        for f in range(2):
            gt = torch.from_numpy(g[f'kitti{d}_gt16_{f}'] / 256).to(dev)
            k = slope_class(gt, pe32, 1.65, 'round').cpu().numpy()
            assert np.array_equal(k.astype(np.float64), g[f'kitti{d}_k_{f}']), int((k != g[f'kitti{d}_k_{f}']).sum())
    for i, cam in enumerate(('CAMERA_01', 'CAMERA_05', 'CAMERA_06', 'CAMERA_09')):
        ref = g[f'ddad{i}_pe']
        H, W = ref.shape
        row2, num = pp_ddad.plane_coefficients(g[f'ddad{i}_K'], g[f'ddad{i}_pose'], g['ddad_lidar_pose'])
        pe64, _ = ground_plane(row2, num, H, W, device=dev)
        assert np.array_equal(pe64.cpu().numpy(), ref)
        k = slope_class_ddad(torch.from_numpy(g[f'ddad{i}_gt']).to(dev), pe64, pp_ddad.CAMERA_HEIGHTS[cam]).cpu().numpy()
        assert np.array_equal(k.astype(np.int64), g[f'ddad{i}_k']), int((k != g[f'ddad{i}_k']).sum())


# ===================================================================== channels-last (NHWC) kernel variants
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('geom', [(2, 64, 12, 20), (3, 96, 7, 9), (2, 512, 4, 6), (1, 1536, 2, 3), (2, 8, 33, 17)])
def test_nhwc_bn_act_bias_act_bilinear_match_nchw(dev, dtype, geom):
    """csrc/nhwc.hip against the NCHW kernels of the same ops (which are pinned to ATen / the oracle above): training-mode
    BatchNorm + ReLU (column statistics), conv bias + LeakyReLU (bias gradient = column sums), bilinear resize both ways;
    forward, every gradient and the running statistics, on the same values stored channels-last."""
    from gedepth_amd import kernels
    from gedepth_amd.kernels import bias_act_, bilinear_resize, bn_act
    B, C, H, W = geom
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = gen(B * 100 + C + H)
    x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.3).to(td)
    go = torch.randn(B, C, H, W, generator=g).to(td)
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == 'bf16' else dict(rtol=1e-4, atol=1e-5)

    def bn_run(cl):
        bn = torch.nn.BatchNorm2d(C).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
        xi = x.to(dev)
        xi = (_cl(xi) if cl else xi).requires_grad_(True)
        if cl and not kernels._cl_ok(xi):
            pytest.skip('channel count outside the NHWC kernels (falls back to NCHW by design)')
        y = bn_act(xi, bn, 0.0)
        assert kernels._is_cl(y) == cl
        y.backward(_cl(go.to(dev)) if cl else go.to(dev))
        return [t.float().cpu() for t in (y, xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)]
    for a, b, n in zip(bn_run(True), bn_run(False), ('y', 'dx', 'dgamma', 'dbeta', 'running_mean', 'running_var')):
        if n in ('dgamma', 'dbeta'):
            close_scaled(a, b, rel=2e-2 if dtype == 'bf16' else 1e-4, what=f'bn_act nhwc {n}')
        else:
            close(a, b, what=f'bn_act nhwc {n}', **tol)

    def bias_run(cl):
        bias = torch.linspace(-1, 1, C, device=dev).requires_grad_(True)
        xi = x.to(dev)
        xi = (_cl(xi) if cl else xi).requires_grad_(True)
        y = bias_act_(xi * 1.0, bias, 0.01)
        assert kernels._is_cl(y) == cl
        y.backward(_cl(go.to(dev)) if cl else go.to(dev))
        return [t.float().cpu() for t in (y, xi.grad, bias.grad)]
    for a, b, n in zip(bias_run(True), bias_run(False), ('y', 'dx', 'dbias')):
        (close_scaled(a, b, rel=2e-2 if dtype == 'bf16' else 1e-4, what=f'bias_act nhwc {n}') if n == 'dbias'
         else close(a, b, what=f'bias_act nhwc {n}', **tol))

    for size, align in (((2 * H, 2 * W), True), ((2 * H, 2 * W), False), ((max(1, H // 2), max(1, W // 2)), True), ((3 * H + 1, 2 * W - 1), False),
                        ((16 * H, 16 * W), True), ((5 * H + 2, 4 * W), False)):          # factors > 3: the separable two-pass backward
        def bil_run(cl):
            xi = x.to(dev)
            xi = (_cl(xi) if cl else xi).requires_grad_(True)
            y = bilinear_resize(xi, size, align)
            assert not cl or kernels._is_cl(y) or y.shape[2] * y.shape[3] == 1
            gy = torch.randn(y.shape, generator=gen(5)).to(td).to(dev)
            y.backward(_cl(gy) if cl else gy)
            return y.float().cpu(), xi.grad.float().cpu()
        (ya, ga), (yb, gb) = bil_run(True), bil_run(False)
        close(ya, yb, what=f'bilinear nhwc fwd {size} ac={align}', **tol)
        close_scaled(ga, gb, rel=2e-2 if dtype == 'bf16' else 1e-4, what=f'bilinear nhwc bwd {size} ac={align}')


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('tokens_first', [True, False])
def test_nhwc_token_map_glue_matches_nchw(dev, dtype, tokens_first):
    """tokens_from_map (a view + the position add) and concat_tokens_map (row concatenation with dropout-free residual) on
    channels-last maps against the transposing NCHW kernels; with dropout the two paths draw different masks, so that case
    checks the statistics and the forward / backward mask consistency instead."""
    from gedepth_amd import kernels
    from gedepth_amd.kernels import concat_tokens_map, tokens_from_map
    B, C, Cm, H, W = 2, 64, 24, 6, 10
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = gen(31)
    fmap = torch.randn(B, C, H, W, generator=g).to(td)
    pos = torch.randn(1, C, H, W, generator=g)
    tokens = torch.randn(B, 3 * H * W, C, generator=g).to(td)[:, H * W:2 * H * W]      # a token range of a longer sequence
    skip = torch.randn(B, Cm, H, W, generator=g).to(td)
    go_t = torch.randn(B, H * W, C, generator=g).to(td)
    go_m = torch.randn(B, C + Cm, H, W, generator=g).to(td)
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == 'bf16' else dict(rtol=1e-5, atol=1e-6)

    def run(cl):
        f = fmap.to(dev)
        f = (_cl(f) if cl else f).requires_grad_(True)
        t = tokens_from_map(f, pos.to(dev))
        t.backward(go_t.to(dev))
        tk = tokens.to(dev).requires_grad_(True)                       # batch-strided rows
        sk = skip.to(dev)
        sk = (_cl(sk) if cl else sk).requires_grad_(True)
        idt = fmap.to(dev)
        idt = (_cl(idt) if cl else idt).requires_grad_(True)
        out = concat_tokens_map(tk, sk, identity=idt, tokens_first=tokens_first, p_drop=0.0)
        assert kernels._is_cl(out) == cl
        out.backward(_cl(go_m.to(dev)) if cl else go_m.to(dev))
        return [v.float().cpu() for v in (t, f.grad, out, tk.grad, sk.grad, idt.grad)]
    for a, b, n in zip(run(True), run(False), ('tokens', 'd map', 'concat', 'd tokens', 'd skip', 'd identity')):
        close(a, b, what=f'nhwc glue {n}', **tol)
    # dropout: E[out] preserved, dropped positions get zero gradient, kept ones 1 / (1 - p)
    tk = torch.ones(B, H * W, C, device=dev, dtype=td, requires_grad=True)
    sk = _cl(torch.zeros(B, Cm, H, W, device=dev, dtype=td))
    out = concat_tokens_map(tk, sk, tokens_first=tokens_first, p_drop=0.25, seed=1234)
    part = out[:, :C] if tokens_first else out[:, Cm:]
    vals = part.float().unique().tolist()
    assert all(v == 0.0 or abs(v - 1 / 0.75) < 1e-2 for v in vals) and abs(part.float().mean().item() - 1.0) < 0.05
    out.sum().backward()
    assert torch.equal((tk.grad.float() > 0), (part.permute(0, 2, 3, 1).reshape(B, H * W, C).float() > 0))


@pytest.mark.gpu
@pytest.mark.parametrize('R,C,dt', [(197120, 96, 'bf16'), (3080, 3072, 'bf16'), (1001, 2304, 'bf16'), (777, 100, 'f32'), (5, 8, 'bf16'),
                                     (49280, 1536, 'f32'), (33, 4104, 'bf16')])
def test_colsum_vs_float64(dev, R, C, dt):
    """Bias gradient of the token Linears: column sums in one pass, fp32 per thread + fp64 across workgroups."""
    from gedepth_amd import kernels
    dtype = torch.bfloat16 if dt == 'bf16' else torch.float32
    x = (torch.randn(R, C, device=dev) * 3 + 0.25).to(dtype)
    got = kernels.colsum(x)
    ref = x.double().sum(0)
    scale = x.double().abs().sum(0)
    assert got.dtype == torch.float32 and got.shape == (C,)
    assert float(((got.double() - ref).abs() / scale).max()) < 2e-6
    assert not [k for k in kernels.FALLBACKS if k.startswith('colsum')]


@pytest.mark.gpu
def test_fused_adamw_bf16_shadow_tracks_parameters(dev):
    """The optimizer kernel writes the bf16 copy the autocast forward reads; ``lowp`` serves it only while it is current."""
    from gedepth_amd.mmrt.optim import FusedAdamW, lowp
    torch.manual_seed(3)
    ps = [torch.randn(s, device=dev).requires_grad_(True) for s in ((33, 7), (129,), (4, 3, 3, 3))]
    opt = FusedAdamW([dict(params=ps, weight_decay=0.01)], lr=1e-2, max_grad_norm=1.0)
    for p in ps:                                                 # built at construction
        assert lowp(p, torch.bfloat16).data_ptr() == p._ge_lp.data_ptr()
        assert torch.equal(p._ge_lp, p.detach().to(torch.bfloat16))
        assert lowp(p, torch.float32) is p
    for _ in range(3):
        for p in ps:
            p.grad.copy_(torch.randn_like(p))
        opt.step()
    for p in ps:
        got = lowp(p, torch.bfloat16)
        assert got.data_ptr() == p._ge_lp.data_ptr() and torch.equal(got, p.detach().to(torch.bfloat16))
    with torch.no_grad():
        ps[0].copy_(torch.ones_like(ps[0]))                      # a foreign write (checkpoint load): the shadow is stale ...
    stale = lowp(ps[0], torch.bfloat16)
    assert stale.data_ptr() != ps[0]._ge_lp.data_ptr() and bool((stale == 1).all())      # ... so a cast is served
    ps[0].grad.zero_()
    opt.step()                                                   # the next step makes it current again
    assert lowp(ps[0], torch.bfloat16).data_ptr() == ps[0]._ge_lp.data_ptr()
    assert torch.equal(ps[0]._ge_lp, ps[0].detach().to(torch.bfloat16))
    plain = FusedAdamW([dict(params=[torch.randn(5, device=dev).requires_grad_(True)])], lr=1e-2, bf16_shadow=False)
    assert getattr(plain.arena, 'flat_shadow', None) is None


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('R,C', [(777, 384), (12320, 1536), (5, 8), (1001, 3072)])
def test_bias_gelu_epilogue(dev, dtype, R, C):
    """ge_bias_gelu_fwd / _bwd (bias + exact-erf GELU epilogue of the FFN's first Linear, depthformer_swin.py:451-459) against
    float64 torch: out = gelu(x + b); dy = dg * gelu'(x + b); d_bias = column sums of dy (of the ROUNDED dy: what the GEMMs read)."""
    from gedepth_amd import kernels
    g = gen(31)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    x = (torch.randn(R, C, generator=g) * 2).to(td)
    b = torch.randn(C, generator=g) * 0.5
    dg = torch.randn(R, C, generator=g).to(td)
    x64 = (x.double() + b.double()).requires_grad_(True)
    ref = F.gelu(x64)
    ref.backward(dg.double())
    out = kernels.bias_gelu_fwd(x.to(dev), b.to(dev))
    dy, db = kernels.bias_gelu_bwd(dg.to(dev), x.to(dev), b.to(dev))
    tol = 1e-2 if dtype == 'bf16' else 2e-6
    close_scaled(out.float(), ref, rel=tol, what='gelu(x + b)')
    close_scaled(dy.float(), x64.grad, rel=tol, what='dy')
    close_scaled(db, dy.float().cpu().double().sum(0), rel=1e-5, what='d_bias = column sums of the stored dy')
    close_scaled(db, x64.grad.sum(0), rel=2e-2 if dtype == 'bf16' else 1e-5, what='d_bias vs float64')


@pytest.mark.gpu
@pytest.mark.parametrize('autocast', [False, True])
def test_ffn_fused_bias_gelu_matches_composition(dev, autocast):
    """mmrt.bricks.FFN with the bias + GELU epilogue kernels against the plain composition F.linear -> F.gelu -> F.linear + identity on
    the same parameters: output and every gradient (fp32: to rounding; bf16 autocast: to bf16 rounding)."""
    from gedepth_amd.mmrt.bricks import FFN
    torch.manual_seed(0)
    ffn = FFN(embed_dims=96, feedforward_channels=384, num_fcs=2, act_cfg=dict(type='GELU'), ffn_drop=0.,
              dropout_layer=dict(type='DropPath', drop_prob=0.)).to(dev).train()
    x = torch.randn(2, 1001, 96, device=dev)
    go = torch.randn(2, 1001, 96, device=dev)
    xa = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        assert ffn._fused_first()
        out = ffn(xa)
    out.backward(go.to(out.dtype))
    got = [out.float(), xa.grad] + [p.grad.clone() for p in ffn.parameters()]
    for p in ffn.parameters():
        p.grad = None
    xb = x.clone().requires_grad_(True)
    l0, l1 = ffn.layers[0][0], ffn.layers[1]
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        ref = xb + F.linear(F.gelu(F.linear(xb, l0.weight, l0.bias)), l1.weight, l1.bias)
    ref.backward(go.to(ref.dtype))
    want = [ref.float(), xb.grad] + [p.grad.clone() for p in ffn.parameters()]
    for a, b, n in zip(got, want, ['out', 'dx', 'dW1', 'db1', 'dW2', 'db2']):
        close_scaled(a.float(), b.float(), rel=2e-2 if autocast else 2e-5, what=f'FFN {n}')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('geom', [(2, 96, 64, (11, 18), (22, 35)), (1, 768, 384, (3, 5), (6, 9)), (2, 8, 8, (5, 7), (9, 13)), (2, 16, 24, (1, 2), (2, 3))])
def test_upcat_matches_interpolate_cat(dev, dtype, geom):
    """kernels.upcat (ge_upcat_nhwc_*: the UpSample block's F.interpolate(align_corners=True) -> torch.cat, densedepth_head.py:25-27,
    as one pass into the concat buffer) against torch on the CPU in float64: forward, d_coarse (the transposed interpolation read
    from the concat gradient in place) and d_skip; exact 2x, non-integer factors and a 1-row coarse map."""
    from gedepth_amd import kernels
    N, Cu, Cs, (Hc, Wc), (H, W) = geom
    g = gen(41)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    coarse = torch.randn(N, Cu, Hc, Wc, generator=g).to(td)
    skip = torch.randn(N, Cs, H, W, generator=g).to(td)
    go = torch.randn(N, Cu + Cs, H, W, generator=g).to(td)
    c64, s64 = coarse.double().requires_grad_(True), skip.double().requires_grad_(True)
    ref = torch.cat([F.interpolate(c64, size=(H, W), mode='bilinear', align_corners=True), s64], 1)
    ref.backward(go.double())
    cg = coarse.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sg = skip.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    kernels.PROFILER.enable()
    out = kernels.upcat(cg, sg, align_corners=True)
    out.backward(go.to(dev))
    kernels.PROFILER.disable()
    assert any(r['name'].startswith('upcat_fwd') for r in kernels.PROFILER.summary()) and kernels._is_cl(out)
    tol = 1e-2 if dtype == 'bf16' else 1e-5
    close_scaled(out.float(), ref, rel=tol, what='upcat')
    close_scaled(cg.grad.float(), c64.grad, rel=tol, what='d coarse')
    close_scaled(sg.grad.float(), s64.grad, rel=tol, what='d skip')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_upsum_matches_pe_trunk_composition(dev, dtype):
    """kernels.upsum (ge_upsum_nhwc_fwd: the PE-neck trunk's four align_corners up-samplings + adds in one pass, pemask_neck.py:52-64)
    against float64 torch, forward and the gradient of every map (factors 16, 8, 4, 2: separable and direct transposes)."""
    from gedepth_amd import kernels
    g = gen(43)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    sizes = [(2, 3), (4, 6), (8, 12), (16, 24)]
    H, W, C, N = 32, 48, 64, 2
    coarse = [torch.randn(N, C, h, w, generator=g).to(td) for h, w in sizes]
    fine = torch.randn(N, C, H, W, generator=g).to(td)
    go = torch.randn(N, C, H, W, generator=g).to(td)
    c64 = [t.double().requires_grad_(True) for t in coarse]
    f64 = fine.double().requires_grad_(True)
    ref = f64
    acc = None
    for t in c64:
        u = F.interpolate(t, size=(H, W), mode='bilinear', align_corners=True)
        acc = u if acc is None else acc + u
    ref = acc + f64
    ref.backward(go.double())
    cl = torch.channels_last
    cg = [t.to(dev).contiguous(memory_format=cl).requires_grad_(True) for t in coarse]
    fg = fine.to(dev).contiguous(memory_format=cl).requires_grad_(True)
    kernels.PROFILER.enable()
    out = kernels.upsum(fg, cg, align_corners=True)
    out.backward(go.to(dev))
    kernels.PROFILER.disable()
    assert any(r['name'].startswith('upsum_fwd') for r in kernels.PROFILER.summary())
    tol = 2e-2 if dtype == 'bf16' else 1e-5
    close_scaled(out.float(), ref, rel=tol, what='upsum')
    close_scaled(fg.grad.float(), f64.grad, rel=tol, what='d fine')
    for a, b, s in zip(cg, c64, sizes):
        close_scaled(a.grad.float(), b.grad, rel=tol, what=f'd coarse {s}')


@pytest.mark.gpu
@pytest.mark.parametrize('geom', [(2, 64, 512, 16, 40), (1, 96, 512, 13, 37), (2, 192, 512, 9, 33), (1, 768, 768, 11, 35), (1, 64, 64, 8, 32),
                                  (1, 384, 512, 22, 70), (2, 96, 96, 44, 70), (1, 64, 544, 30, 33)])
def test_conv1x1_wgrad_vs_float64(dev, geom, monkeypatch):
    """ge_conv1x1_nhwc_wgrad (csrc/conv1x1_wgrad.hip: dW = dY^T X streamed over the pixels, MFMA with transposing LDS reads, K split with an
    fp32 atomic flush) against a float64 contraction of the same bf16-rounded operands: row counts that are not multiples of the 64-row
    stage, one / several Cin chunks of 64 and of 96, Cout above 512 (two Cout chunks, the second partial), the HAHI shapes."""
    from gedepth_amd import kernels
    N, Ci, Co, H, W = geom
    g = gen(31)
    cl = torch.channels_last
    x = torch.randn(N, Ci, H, W, generator=g).bfloat16().to(dev).contiguous(memory_format=cl)
    dy = torch.randn(N, Co, H, W, generator=g).bfloat16().to(dev).contiguous(memory_format=cl)
    w = torch.empty(Co, Ci, 1, 1, device=dev, dtype=torch.bfloat16)
    monkeypatch.setattr(kernels, 'ENABLED', kernels.ENABLED | {'conv1x1_wgrad'})          # opt-in path (measured slower than the library: kernels.conv1x1_wgrad_ok)
    assert kernels.conv1x1_wgrad_ok(x, dy, w, (1, 1), (0, 0), (1, 1), 1) == (N * H * W >= 2048)
    dw = kernels.conv1x1_wgrad(x, dy)
    ref = torch.einsum('nohw,nihw->oi', dy.double(), x.double())
    close_scaled(dw, ref, rel=2e-5, what=f'conv1x1 wgrad {geom}')


@pytest.mark.gpu
def test_conv_module_1x1_opt_in_wgrad_matches_library(dev, monkeypatch):
    """A ConvModule(k = 1)-style convolution under bf16 autocast through kernels.conv_lib with the opt-in GE_ENABLE=conv1x1_wgrad: the weight
    gradient comes from ge_conv1x1_nhwc_wgrad (profiler record) and equals the library's (the default) to fp32-accumulation accuracy; dx unchanged."""
    from gedepth_amd import kernels
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(64, 512, 1, bias=False).to(dev).to(memory_format=torch.channels_last)
    x0 = torch.randn(2, 64, 40, 56, device=dev).contiguous(memory_format=torch.channels_last)
    go = torch.randn(2, 512, 40, 56, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)

    def run():
        x = x0.clone().requires_grad_(True)
        conv.weight.grad = None
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = kernels.conv_lib(conv, x)
        y.backward(go)
        return y.float(), x.grad.float(), conv.weight.grad.float().clone()
    monkeypatch.setattr(kernels, 'ENABLED', kernels.ENABLED | {'conv1x1_wgrad'})
    kernels.PROFILER.enable()
    y1, dx1, dw1 = run()
    kernels.PROFILER.disable()
    assert any(r['name'].startswith('conv1x1_wgrad') for r in kernels.PROFILER.summary())
    monkeypatch.setattr(kernels, 'ENABLED', kernels.ENABLED - {'conv1x1_wgrad'})
    y2, dx2, dw2 = run()
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    close_scaled(dw1, dw2, rel=1e-2, what='1x1 weight gradient: own (fp32 accumulation) vs library (bf16 result)')


@pytest.mark.gpu
@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('geom', [(2, 64, 64, 16, 40), (1, 160, 64, 13, 37), (2, 96, 96, 9, 33), (1, 288, 192, 22, 70), (1, 64, 128, 8, 32), (2, 32, 32, 3, 5),
                                  (1, 576, 64, 176, 560)])
@pytest.mark.parametrize('variant', ['1', '2'])
def test_conv3x3_mfma_vs_conv2d(dev, geom, act, variant, monkeypatch):
    """kernels.conv3x3 (ge_conv3x3_nhwc_fwd: implicit-GEMM 3x3 convolution on v_mfma_f32_32x32x16_bf16 with the bias + LeakyReLU epilogue;
    its data gradient = the same kernel on flipped / transposed weights; weight gradient = ge_conv3x3_nhwc_wgrad, transposing LDS reads) against F.conv2d in float64 on the
    same bf16-rounded operands: y, d_x, d_w, d_bias; tiles that hang over the right / bottom border, several 64-channel output tiles, a
    partial one (96), maps smaller than one tile, and the largest layer of the bench step (1 x 576 -> 64 @176 x 560: forward, data gradient
    and the K-split weight gradient with its fp32 atomic flush).  Both forward kernels: the register-staged 8 x 32 tile (variant 1) and the
    LDS-DMA 16 x 32 tile (variant 2, round 4) — selected through GE_CONV3X3, which the library reads per call."""
    from gedepth_amd import kernels
    monkeypatch.setenv('GE_CONV3X3', variant)
    N, Ci, Co, H, W = geom
    if H * W > 50000 and act:
        pytest.skip('the bench-shape case runs once per kernel variant (float64 reference on the CPU: ~20 s)')
    g = gen(51)
    x = torch.randn(N, Ci, H, W, generator=g).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).bfloat16()
    b = torch.randn(Co, generator=g) * 0.2
    go = torch.randn(N, Co, H, W, generator=g).bfloat16()
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(x64, w64, b64, padding=1)
    if act:
        ref = F.leaky_relu(ref, 0.01)
    ref.backward(go.double())
    conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(b)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert kernels.conv3x3_ok(conv, xg)
    kernels.PROFILER.enable()
    y = kernels.conv3x3(conv, xg, conv.bias, act=act, slope=0.01)
    y.backward(go.to(dev))
    kernels.PROFILER.disable()
    names = [r['name'] for r in kernels.PROFILER.summary()]
    assert sum(n.startswith('conv3x3[') for n in names) == 2                                      # forward and data gradient on the MFMA kernel
    # the MFMA weight gradient is used from 1e4 pixels (where it beats MIOpen); checked here directly at every geometry
    dw = torch.zeros(Co, 3, 3, Ci, device=dev)
    from gedepth_amd import hip
    xb, gb = xg.detach(), go.to(dev).contiguous(memory_format=torch.channels_last)
    dyp = gb if not act else (gb.float() * torch.where(y.detach().float() > 0, 1.0, 0.01)).bfloat16().contiguous(memory_format=torch.channels_last)
    hip.check(hip.lib().ge_conv3x3_nhwc_wgrad(xb.data_ptr(), dyp.data_ptr(), dw.data_ptr(), N, H, W, Ci, Co, 1, hip.stream()), 'ge_conv3x3_nhwc_wgrad')
    close_scaled(dw.permute(0, 3, 1, 2), w64.grad, rel=2e-2, what='ge_conv3x3_nhwc_wgrad')
    # fp32 accumulation of exact bf16 x bf16 products: every element (l2-relative) to 1e-3; with the activation the incoming gradient is
    # itself rounded to bf16 after the LeakyReLU mask (what the backward of the convolution receives), which the float64 reference does not do
    e_dw = l2rel(dw.permute(0, 3, 1, 2), w64.grad)
    assert e_dw <= (1e-3 if not act else 4e-3), f'ge_conv3x3_nhwc_wgrad l2-relative error {e_dw:.2e}'
    assert y.dtype == torch.bfloat16 and kernels._is_cl(y)
    close_scaled(y.float(), ref, rel=1e-2, what='conv3x3 y')
    close_scaled(xg.grad.float(), x64.grad, rel=1e-2, what='conv3x3 d_x')
    close_scaled(conv.weight.grad.float(), w64.grad, rel=2e-2, what='conv3x3 d_w')
    close_scaled(conv.bias.grad.float(), b64.grad, rel=2e-2, what='conv3x3 d_bias')


@pytest.mark.parametrize('geom', [(8, 64, 176, 560), (2, 64, 13, 37), (1, 72, 9, 5), (3, 128, 1, 1), (1, 8, 40, 33)])
@pytest.mark.parametrize('out_fp32', [False, True])
def test_conv3x3_one_output_channel_vs_conv2d(dev, geom, out_fp32):
    """kernels.conv3x3_c1 (ge_conv3x3_c1_fwd / _bwd: the 64 -> 1 depth regressor and ground-attention head as a streaming reduction;
    ONE backward pass for d_x, d_w, d_bias) against F.conv2d in float64 on the same bf16-rounded operands: the bench shape, maps smaller
    than a wave's 8 pixels, channel counts that are not a multiple of 64 (72: the last 8-lane step is partly masked; 128: two steps)."""
    from gedepth_amd import kernels
    N, Ci, H, W = geom
    g = gen(52)
    x = torch.randn(N, Ci, H, W, generator=g).bfloat16()
    w = (torch.randn(1, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).bfloat16()
    b = torch.randn(1, generator=g) * 0.2
    go = torch.randn(N, 1, H, W, generator=g)
    if not out_fp32:
        go = go.bfloat16()
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(x64, w64, b64, padding=1)
    ref.backward(go.double())
    conv = torch.nn.Conv2d(Ci, 1, 3, padding=1).to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(b)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert kernels.conv3x3_c1_ok(conv, xg)
    kernels.PROFILER.enable()
    y = kernels.conv3x3_c1(conv, xg, out_fp32=out_fp32)
    y.backward(go.to(dev))
    kernels.PROFILER.disable()
    names = [r['name'] for r in kernels.PROFILER.summary()]
    assert any(n.startswith('conv3x3_c1[') for n in names) and any(n.startswith('conv3x3_c1_bwd[') for n in names)
    assert y.dtype == (torch.float32 if out_fp32 else torch.bfloat16) and y.shape == (N, 1, H, W)
    close_scaled(y.float(), ref, rel=1e-2 if not out_fp32 else 2e-5, what='conv3x3_c1 y')
    close_scaled(xg.grad.float(), x64.grad, rel=1e-2, what='conv3x3_c1 d_x')
    assert conv.weight.grad.shape == (1, Ci, 3, 3)
    close_scaled(conv.weight.grad.float(), w64.grad, rel=1e-4, what='conv3x3_c1 d_w')
    close_scaled(conv.bias.grad.float(), b64.grad, rel=1e-4, what='conv3x3_c1 d_bias')


def test_residual_dropout_and_add_rows(dev):
    """kernels.residual_dropout (identity + dropout(tokens): forward mask recomputed in backward from the seed) and kernels.add_rows
    (tokens + fp32 rows broadcast over the batch, gradient to the rows = batch sum) — the self-attention glue of the HAHI neck."""
    from gedepth_amd import kernels
    g = gen(53)
    B, N, C, p = 3, 517, 64, 0.25
    tok = torch.randn(B, N, C, generator=g).bfloat16().to(dev).requires_grad_(True)
    idt = torch.randn(B, N, C, generator=g).bfloat16().to(dev).requires_grad_(True)
    # the mask is a function of (seed, element index): read it off a call with a zero identity
    with torch.no_grad():
        plain = kernels.residual_dropout(torch.zeros_like(idt), tok, p, seed=1234).float()
    kept = (tok.detach().float() / (1 - p)).bfloat16().float()
    dropped = (plain == 0) & (kept != 0)
    assert 0.2 < dropped.float().mean().item() < 0.3
    assert torch.equal(torch.where(dropped, torch.zeros_like(kept), kept), plain)
    out = kernels.residual_dropout(idt, tok, p, seed=1234)
    assert torch.equal(out, (plain + idt.detach().float()).bfloat16())                         # dropout(tokens) is rounded, then added: one more rounding
    diff = out.float() - idt.float()
    go = torch.randn(B, N, C, generator=g).bfloat16().to(dev)
    out.backward(go)
    close_scaled(idt.grad.float(), go.float(), rel=1e-6, what='d_identity')
    want = torch.where(dropped, torch.zeros_like(diff), go.float() / (1 - p))
    close_scaled(tok.grad.float(), want, rel=1e-2, what='d_tokens uses the forward mask')
    out2 = kernels.residual_dropout(idt, tok, p, seed=1234)
    assert torch.equal(out2, out)                                              # same seed, same mask
    # add_rows with a gradient for the rows
    rows = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    t2 = tok.detach().clone().requires_grad_(True)
    y = kernels.add_rows(t2, rows)
    ref = (t2.detach().float() + rows.detach()[None]).bfloat16()
    assert torch.equal(y, ref)
    y.backward(go)
    close_scaled(t2.grad.float(), go.float(), rel=1e-6, what='add_rows d_tokens')
    close_scaled(rows.grad, go.float().sum(0), rel=1e-5, what='add_rows d_rows')


def test_conv_lib_reads_the_bf16_shadow(dev):
    """kernels.conv_lib: the library convolution fed from the optimizer's bf16 shadow weight gives the gradients of the plain autocast
    convolution (same library kernels, the weight cast is the only thing removed)."""
    from gedepth_amd import kernels
    from gedepth_amd.mmrt.optim import FusedAdamW
    g = gen(54)
    conv = torch.nn.Conv2d(24, 40, 1, bias=False).to(dev).to(memory_format=torch.channels_last)
    conv2 = torch.nn.Conv2d(16, 8, 3, stride=2, padding=1, bias=False).to(dev).to(memory_format=torch.channels_last)
    opt = FusedAdamW(list(conv.parameters()) + list(conv2.parameters()), lr=1e-3)
    assert getattr(conv.weight, '_ge_lp', None) is not None
    for c, x in ((conv, torch.randn(2, 24, 9, 11, generator=g)), (conv2, torch.randn(2, 16, 10, 14, generator=g))):
        x1 = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        x2 = x1.detach().clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y1 = kernels.conv_lib(c, x1)
            y2 = c(x2)
        assert y1.dtype == torch.bfloat16 and torch.equal(y1, y2)
        go = torch.randn_like(y1)
        y1.backward(go)
        g1 = c.weight.grad.clone()
        c.weight.grad = None
        y2.backward(go)
        assert g1.dtype == torch.float32
        close_scaled(g1, c.weight.grad, rel=1e-6, what='conv_lib d_w')
        close_scaled(x1.grad, x2.grad, rel=1e-6, what='conv_lib d_x')


@pytest.mark.parametrize('dtypes', ['f32->bf16', 'bf16->bf16', 'f32->f32'])
def test_layer_norm_with_skip_gradient(dev, dtypes):
    """kernels.layer_norm_res: (LN(x), x') — the gradient arriving over the skip output is added inside ge_layernorm_bwd_res; against
    LayerNorm + residual in float64 (the pre-norm block pattern of the Swin encoder), and against the two-kernel composition."""
    from gedepth_amd import kernels
    tx, ty = (torch.float32 if t == 'f32' else torch.bfloat16 for t in dtypes.split('->'))
    g = gen(55)
    B, N, C = 3, 211, 96
    x = torch.randn(B, N, C, generator=g).to(tx)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    go_y, go_s = torch.randn(B, N, C, generator=g).to(ty), torch.randn(B, N, C, generator=g).to(tx)
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = F.layer_norm(x64, (C,), w64, b64, 1e-5)
    (y64 * go_y.double()).sum().backward(retain_graph=True)
    (x64 * go_s.double()).sum().backward()
    xg = x.to(dev).requires_grad_(True)
    wg, bg = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    kernels.PROFILER.enable()
    y, xs = kernels.layer_norm_res(xg, wg, bg, 1e-5, ty)
    torch.autograd.backward([y, xs], [go_y.to(dev), go_s.to(dev)])
    kernels.PROFILER.disable()
    assert any('+res' in r['name'] for r in kernels.PROFILER.summary())
    assert torch.equal(xs, xg)
    tol = 2e-2 if torch.bfloat16 in (tx, ty) else 1e-5
    close_scaled(y.float(), y64, rel=tol, what='y')
    close_scaled(xg.grad.float(), x64.grad, rel=tol, what='d_x = LN bwd + skip')
    close_scaled(wg.grad, w64.grad, rel=tol, what='d_gamma')
    close_scaled(bg.grad, b64.grad, rel=tol, what='d_beta')
    # skip output unused -> plain backward; LN output unused -> pass-through
    x2 = x.to(dev).requires_grad_(True)
    y2, _ = kernels.layer_norm_res(x2, wg, bg, 1e-5, ty)
    y2.backward(go_y.to(dev))
    x3 = x.to(dev).requires_grad_(True)
    y3 = kernels.layer_norm(x3, wg, bg, 1e-5, ty)
    y3.backward(go_y.to(dev))
    assert torch.equal(x2.grad, x3.grad)
    x4 = x.to(dev).requires_grad_(True)
    _, s4 = kernels.layer_norm_res(x4, wg, bg, 1e-5, ty)
    s4.backward(go_s.to(dev))
    assert torch.equal(x4.grad, go_s.to(dev))


# ------------------------------------------------------------------------------ token GEMM (csrc/gemm.hip)
@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(49280, 192, 192), (12320, 384, 1152), (1000, 520, 264), (257, 72, 8), (256, 64, 256), (255, 8, 8),
                                   (3080, 3072, 768), (70000, 96, 288), (513, 136, 520)])
@pytest.mark.parametrize('with_bias', [True, False])
def test_gemm_nt_vs_float64(dev, shape, with_bias):
    """ge_gemm_nt = F.linear on bf16 operands: every output element against float64 on the same bf16-rounded operands (one rounding of the
    fp32 sum: 2^-9 relative + the fp32 accumulation error), M / N / K tails (M % 256, N % 256, K % 64 != 0), two launches bit-identical."""
    from gedepth_amd import kernels
    M, K, N = shape
    g = torch.Generator(device='cpu').manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g).to(dev) if with_bias else None
    y = kernels.gemm_nt(x, w, b)
    ref = x.double() @ w.double().t()
    if with_bias:
        ref = ref + b.double()
    err = (y.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-2 * (K ** 0.5) * 2.0 ** -12 + 1e-6
    bad = ~(err <= tol)                      # NaN-strict, like close()
    assert not bool(bad.any()), (shape, int(bad.sum()), f'{int((~torch.isfinite(y)).sum())} non-finite', float(err.nan_to_num(nan=float('inf')).max()))
    assert torch.equal(y, kernels.gemm_nt(x, w, b))
    # padding rows / columns of the last tiles must not leak: a sentinel-framed output buffer stays intact
    from gedepth_amd import hip
    buf = torch.full((M + 2, N), 7.0, device=dev, dtype=torch.bfloat16)
    rc = hip.lib().ge_gemm_nt(x.data_ptr(), K, w.data_ptr(), K, None if b is None else b.data_ptr(), buf[1:M + 1].data_ptr(), N, M, N, K,
                              hip.GE_BF16, hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[1:M + 1], y) and bool((buf[0] == 7).all()) and bool((buf[M + 1] == 7).all())


@pytest.mark.gpu
def test_gemm_nt_refuses_what_it_does_not_cover(dev):
    from gedepth_amd import hip
    x = torch.zeros(64, 64, device=dev, dtype=torch.bfloat16)
    y = torch.zeros(64, 64, device=dev, dtype=torch.bfloat16)
    lib, st = hip.lib(), hip.stream()
    assert lib.ge_gemm_nt(x.data_ptr(), 64, x.data_ptr(), 64, None, y.data_ptr(), 64, 64, 64, 64, hip.GE_F32, st) == 10002      # fp32 storage
    assert lib.ge_gemm_nt(x.data_ptr(), 64, x.data_ptr(), 64, None, y.data_ptr(), 64, 64, 60, 64, hip.GE_BF16, st) == 10002     # N % 8
    assert lib.ge_gemm_nt(x.data_ptr(), 64, x.data_ptr(), 64, None, y.data_ptr(), 64, 64, 64, 60, hip.GE_BF16, st) == 10002     # K % 8
    assert lib.ge_gemm_nt(x.data_ptr() + 2, 64, x.data_ptr(), 64, None, y.data_ptr(), 64, 32, 64, 64, hip.GE_BF16, st) == 10002  # alignment
    assert lib.ge_gemm_nt(None, 64, x.data_ptr(), 64, None, y.data_ptr(), 64, 64, 64, 64, hip.GE_BF16, st) == 10001
    assert lib.ge_gemm_nt(x.data_ptr(), 64, x.data_ptr(), 64, None, y.data_ptr(), 64, 0, 64, 64, hip.GE_BF16, st) == 0          # empty: no launch


@pytest.mark.gpu
@pytest.mark.parametrize('gelu', [False, True])
def test_token_linear_on_own_gemm_matches_library_path(dev, gelu, monkeypatch):
    """bricks.linear_tokens / linear_bias_gelu with every GEMM routed through ge_gemm_nt (forward and input gradient) against the same
    module on the library GEMMs and against float64 autograd on the bf16-rounded operands."""
    from gedepth_amd import kernels
    from gedepth_amd.mmrt import bricks
    torch.manual_seed(5)
    M, K, N = 9000, 96, 288
    x0 = torch.randn(3, M // 3, K, device=dev)
    lin = torch.nn.Linear(K, N).to(dev)
    dy = torch.randn(3, M // 3, N, device=dev).to(torch.bfloat16)

    def run(own):
        monkeypatch.setattr(kernels, '_GEMM_ALL', own)
        monkeypatch.setattr(kernels, 'GEMM_OWN', {} if not own else kernels.GEMM_OWN)
        x = x0.clone().requires_grad_(True)
        lin.zero_grad()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = bricks.linear_bias_gelu(x, lin.weight, lin.bias) if gelu else bricks.linear_tokens(x, lin.weight, lin.bias)
        y.backward(dy)
        return y.detach(), x.grad.detach(), lin.weight.grad.detach().clone(), lin.bias.grad.detach().clone()
    own, libp = run(True), run(False)
    xd = x0.to(torch.bfloat16).double().requires_grad_(True)
    wd = lin.weight.detach().to(torch.bfloat16).double().requires_grad_(True)
    bd = lin.bias.detach().double().requires_grad_(True)
    yd = F.linear(xd, wd, bd)
    if gelu:
        yd = F.gelu(yd)
    yd.backward(dy.double())
    ref = (yd.detach(), xd.grad, wd.grad, bd.grad)
    for name, a, l, r in zip(('y', 'dx', 'dw', 'db'), own, libp, ref):
        scale = float(r.abs().max())
        e_own, e_lib = float((a.double() - r).abs().max()) / scale, float((l.double() - r).abs().max()) / scale
        assert e_own <= max(1.5 * e_lib, 2.0 ** -7), (name, e_own, e_lib)
