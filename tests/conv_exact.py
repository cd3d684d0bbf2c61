"""Exact arithmetic for the convolution kernels (imported like ``f64ref``; used by test_conv_exact_cpu.py and test_conv_exact_gpu.py).

With small INTEGER-valued bf16 operands every product is exact, and as long as the sum of the |products| of one output stays below 2^24 every
partial sum is an integer (or, with the slope 0.5, a multiple of 0.5 below 2^23) that fp32 holds exactly — in ANY order: MFMA, v_dot2, the
split-K and per-workgroup fp32 atomics.  So a kernel's result must EQUAL the float64 reference: fp32 outputs as they are, bf16 outputs after
one round-to-nearest-even.  No tolerance: a dropped, duplicated or misplaced term, or a truncation instead of a rounding, fails.

Everything here runs on the CPU; the cases are built once per process (``functools.lru_cache``) and must be left unchanged by their users.
Activation slopes are exact in binary: ``None`` (no activation), 0.0 (ReLU), 0.5.  Pre-activations that are exactly 0 are common with integer
data: the kernels' mask (``y > 0 ? 1 : slope``) and torch's leaky_relu / relu backward (``x > 0 ? g : g * slope``) agree on "slope at 0"."""
import collections
import functools

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
LIMIT = float(1 << 24)
# integer ranges [-v, v] of the operands.  x, dy and w are stored in bf16; the bias and the master weights in fp32
RANGES = dict(x=4, w=3, b=8, dy=4)
# cases whose base ranges fall short of the rounding conditions (``_assert_rounding_exercised``) or of the 2^24 bound: widened / narrowed here,
# never the thresholds.  Key: (kind, geometry, slope); measured on the CPU by test_conv_exact_cpu.py, which asserts the conditions for every case
RANGE_OVERRIDES = {}

NCHW = ('n', 'channel', 'y', 'x')
OIRS = ('co', 'ci', 'r', 's')
OI = ('co', 'ci')

# --------------------------------------------------------------------------------------------------------------------------- the cases
# kernels.conv3x3 through autograd, and ge_conv3x3_nhwc_wgrad called directly at the same shapes: (N, Cin, Cout, H, W)
#   (2,96,96,9,33)  three K chunks (the prefetch steady state), a partial 64-channel Cout tile, one tile row / column over the border (8-row tile)
#   (2,96,96,17,33) the same for the 16-row LDS-DMA tile
#   (1,32,32,1,1), (2,32,64,2,31) maps smaller than a tile and smaller than the halo
CONV3X3_GEOMS = ((2, 96, 96, 9, 33), (2, 96, 96, 17, 33), (1, 32, 32, 1, 1), (2, 32, 64, 2, 31), (1, 160, 64, 13, 37))
SLOPES = (None, 0.0, 0.5)
CONV3X3_WGRAD_MULTI_TILE = (7, 512, 128, 9, 97)          # 56 tiles of 8 x 32 for 32 output blocks: workgroups walk 3 or 4 tiles on 256 CUs
CONV3X3_WGRAD_AUTOGRAD = (1, 32, 64, 100, 101)           # 10 100 pixels: at the 10 000-pixel threshold of _Conv3x3.backward
for _g in CONV3X3_GEOMS + (CONV3X3_WGRAD_MULTI_TILE, CONV3X3_WGRAD_AUTOGRAD):
    # ReLU zeroes half of the gradient: with dy in [-4, 4] only 0.1 - 0.7 % of dx at Cin >= 96 is not representable in bf16; [-8, 8] gives 3 - 6 %
    RANGE_OVERRIDES[('conv3x3', _g, 0.0)] = dict(dy=8)
CONV3X3_ABI_COUTS = (40, 72)                            # Cout % 8 == 0 but not % 32: the last 16-byte pieces of a tile are cut
CONV3X3_ABI_GEOM = (2, 64, 9, 33)                        # (N, Cin, H, W)
# kernels.conv3x3_c1: (N, Cin, H, W); the last two make a workgroup walk more than one unit of 4 rows x 128 pixels (backward grid: 1024
# workgroups, forward grid: 4096)
C1_GEOMS = ((2, 64, 13, 37), (1, 72, 9, 5), (3, 128, 1, 1), (1, 8, 40, 33))
C1_MULTI_UNIT_BWD = (5, 8, 413, 129)                     # 1040 units
C1_MULTI_UNIT_FWD = (8, 8, 413, 513)                     # 4160 units
C1_XSEG, C1_ROWS, C1_CAP_FWD, C1_CAP_BWD = 128, 4, 4096, 1024          # csrc/conv3x3_c1.hip: C1_XSEG, rows per unit, c1_grid() caps
RANGE_OVERRIDES[('c1', C1_MULTI_UNIT_FWD)] = dict(dy=2)  # 1.7e6 pixels: N H W max|x| max|dy| must stay below 2^24 for d_w
# kernels.conv1x1_wgrad: Cin 64 / 192 = the 64- and 96-channel chunks; Cout 544 = a second Cout chunk that holds a single 32-block
CONV1X1_CIN, CONV1X1_COUT = (64, 192), (32, 544)
CONV1X1_STAGE, CONV1X1_CO_CHUNK = 64, 512                # csrc/conv1x1_wgrad.hip: C1_ROWS, C1_MAX_CB * 32


def c1_units(N, H, W):
    return N * ((H + C1_ROWS - 1) // C1_ROWS) * ((W + C1_XSEG - 1) // C1_XSEG)


def conv3x3_wgrad_split(geom, cus):
    """(tiles, ksplit) of ge_conv3x3_nhwc_wgrad's launcher: 8 x 32 pixel tiles, ksplit = min(2 CUs / output blocks, tiles), at least 1."""
    N, Ci, Co, H, W = geom
    tiles = N * ((H + 7) // 8) * ((W + 31) // 32)
    blocks_out = (Ci // 32) * ((Co + 63) // 64)
    return tiles, max(1, min(2 * cus // blocks_out, tiles))


def conv1x1_wgrad_split(M, Ci, Co, cus):
    """(stages, ksplit) of ge_conv1x1_nhwc_wgrad's launcher: 64-row stages, ksplit = min(CUs / (n_ci n_co), stages), at least 1."""
    n_ci = Ci // (96 if Ci % 96 == 0 else 64)
    n_co = (Co + CONV1X1_CO_CHUNK - 1) // CONV1X1_CO_CHUNK
    stages = (M + CONV1X1_STAGE - 1) // CONV1X1_STAGE
    return stages, max(1, min(cus // (n_ci * n_co), stages, 65535))


def conv1x1_rows(Ci, Co, cus):
    """The two row counts of a conv1x1_wgrad case: at least 3 stages per workgroup plus a ragged last stage, and 2048 + 5."""
    n_ci = Ci // (96 if Ci % 96 == 0 else 64)
    n_co = (Co + CONV1X1_CO_CHUNK - 1) // CONV1X1_CO_CHUNK
    return CONV1X1_STAGE * 3 * (cus // (n_ci * n_co)) + 37, 2048 + 5


# ------------------------------------------------------------------------------------------------------------------------ operands
def ints(g, shape, lim, dtype=torch.float32):
    """Integer-valued tensor, uniform on [-lim, lim], from the seeded CPU generator ``g``."""
    return torch.randint(-lim, lim + 1, shape, generator=g).to(dtype)


def _ranges(key):
    r = dict(RANGES)
    r.update(RANGE_OVERRIDES.get(key, {}))
    return r


def _amax(t):
    return float(t.abs().max()) if t is not None and t.numel() else 0.0


def assert_sums_exact(what, n_y, n_dx, n_dw, x, w, b, dy, half=False):
    """The a-priori bound: the sum of the |products| of one output stays below 2^24 (2^23 where values are multiples of 0.5), so every
    partial sum in fp32 is exact whatever the order.  ``n_*``: number of products per element of y, dx, dW."""
    lim = LIMIT / 2 if half else LIMIT
    mx, mw, mb, md = _amax(x), _amax(w), (_amax(b) if b is not None else 0.0), _amax(dy)
    bounds = {'y': n_y * mx * mw + mb, 'dx': n_dx * md * mw, 'dW': n_dw * mx * md, 'd_bias': n_dw * md,
              'issue': max(n_y, n_dx) * max(mx, md) * mw + mb}
    for k, v in bounds.items():
        assert v < lim, f'{what}: the sum of |products| of one {k} element can reach {v:.0f} >= {lim:.0f}: fp32 sums would not be exact'
    for name, t in (('x', x), ('w', w), ('b', b), ('dy', dy)):
        if t is not None:
            assert torch.equal(t.double(), t.double().round()) and _amax(t) <= 256, f'{what}: {name} is not a small integer tensor'
    return bounds


def rounding_share(ref64):
    """(share of the elements that bf16 cannot represent, number of exact ties) of a float64 reference that fp32 holds exactly.  A tie has
    the fp32 low 16 bits equal to 0x8000: round-to-nearest-even and round-half-away differ there, and truncation differs on all of them."""
    f = ref64.to(torch.float32)
    assert torch.equal(f.double(), ref64.double()), 'the reference is not exact in fp32'
    low = f.contiguous().view(torch.int32) & 0xFFFF
    return float((low != 0).double().mean()), int((low == 0x8000).sum())


def assert_rounding_exercised(what, y64, dx64):
    """bf16 rounding must really happen in the case: >= 1 % of y and of dx not representable in bf16, and at least one exact tie in each."""
    out = {}
    for name, t in (('y', y64), ('dx', dx64)):
        share, ties = rounding_share(t)
        out[name] = (share, ties)
        assert share >= 0.01, f'{what}: only {100 * share:.2f} % of {name} is not representable in bf16 (needs >= 1 %): widen the operand ranges'
        assert ties >= 1, f'{what}: no element of {name} is an exact bf16 tie: widen the operand ranges'
    return out


def truncate_to_bf16(t):
    """fp32-exact tensor -> bf16 by dropping the low 16 bits (what a kernel that forgets to round would store)."""
    f = t.to(torch.float32).contiguous()
    return (f.view(torch.int32) & -65536).view(torch.float32).to(BF16)


def _act(t, slope):
    if slope is None:
        return t
    return F.relu(t) if slope == 0.0 else F.leaky_relu(t, slope)


Conv3x3Case = collections.namedtuple('Conv3x3Case', 'geom slope x w b dy dyp y dx dw db y32 dx32 bounds rounding')


@functools.lru_cache(maxsize=None)
def conv3x3_case(geom, slope):
    """act(conv3x3(x, w) + b) and its gradients in float64 on integer operands.  x, dy bf16 (N, C, H, W); w, b fp32 (the master weight and
    bias; exact in bf16 too).  Expected results in the dtype the kernels store: y, dx bf16 (one round-to-nearest-even of the float64
    reference), dw (Cout, Cin, 3, 3), db fp32.  dyp: the masked, bf16 dy that the backward of the convolution really receives
    (dy * (pre-activation > 0 ? 1 : slope), exact).  y32, dx32: the references before the bf16 rounding (exact in fp32)."""
    N, Ci, Co, H, W = geom
    r = _ranges(('conv3x3', geom, slope))
    g = torch.Generator().manual_seed(1000 + sum(geom) * 3 + (0 if slope is None else 1 + int(slope * 2)))
    x = ints(g, (N, Ci, H, W), r['x'])
    w = ints(g, (Co, Ci, 3, 3), r['w'])
    b = ints(g, (Co,), r['b'])
    dy = ints(g, (N, Co, H, W), r['dy'])
    what = f'conv3x3 {geom} slope {slope}'
    bounds = assert_sums_exact(what, 9 * Ci, 9 * Co, N * H * W, x, w, b, dy, half=slope == 0.5)
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(x64, w64, b64, padding=1)
    y64 = _act(pre, slope)
    y64.backward(dy.double())
    mask = torch.ones_like(pre) if slope is None else torch.where(pre.detach() > 0, 1.0, float(slope)).double()
    dyp = dy.double() * mask
    assert torch.equal(dyp.to(BF16).double(), dyp)                           # the masked gradient is exact in bf16
    y64, dx64 = y64.detach(), x64.grad
    rounding = assert_rounding_exercised(what, y64, dx64) if Ci >= 96 else None
    f32 = torch.float32
    return Conv3x3Case(geom, slope, x.to(BF16), w, b, dy.to(BF16), dyp.to(BF16), y64.to(BF16), dx64.to(BF16), w64.grad.to(f32), b64.grad.to(f32),
                       y64.to(f32), dx64.to(f32), bounds, rounding)


AbiCase = collections.namedtuple('AbiCase', 'geom cout slope x w b dy y dw')


@functools.lru_cache(maxsize=None)
def conv3x3_abi_case(cout, slope=0.5):
    """ge_conv3x3_nhwc_fwd / _wgrad called through the C ABI with a Cout that is a multiple of 8 only: y bf16 (N, Cout, H, W), dw fp32."""
    N, Ci, H, W = CONV3X3_ABI_GEOM
    r = _ranges(('abi', cout))
    g = torch.Generator().manual_seed(2000 + cout)
    x, w, b, dy = ints(g, (N, Ci, H, W), r['x']), ints(g, (cout, Ci, 3, 3), r['w']), ints(g, (cout,), r['b']), ints(g, (N, cout, H, W), r['dy'])
    assert_sums_exact(f'conv3x3 C ABI Cout {cout}', 9 * Ci, 9 * cout, N * H * W, x, w, b, dy, half=True)
    w64 = w.double().requires_grad_(True)
    pre = F.conv2d(x.double(), w64, b.double(), padding=1)
    pre.backward(dy.double())                                                # the weight gradient of the plain convolution for this dy
    y64 = _act(pre.detach(), slope)
    return AbiCase(CONV3X3_ABI_GEOM, cout, slope, x.to(BF16), w.to(BF16), b, dy.to(BF16), y64.to(BF16), w64.grad.to(torch.float32))


C1Case = collections.namedtuple('C1Case', 'geom out_fp32 x w b dy y dx dw db y32')


@functools.lru_cache(maxsize=None)
def c1_case(geom, out_fp32):
    """conv3x3 to ONE output channel (+ bias): y in fp32 (exact) or bf16 (rounded once), dx bf16, dw (1, Cin, 3, 3) and db fp32.  dy has the
    dtype of y, as autograd hands it to the backward."""
    N, Ci, H, W = geom
    r = _ranges(('c1', geom))
    g = torch.Generator().manual_seed(3000 + sum(geom) * 3 + int(out_fp32))
    x, w, b, dy = ints(g, (N, Ci, H, W), r['x']), ints(g, (1, Ci, 3, 3), r['w']), ints(g, (1,), r['b']), ints(g, (N, 1, H, W), r['dy'])
    assert_sums_exact(f'conv3x3_c1 {geom}', 9 * Ci, 9, N * H * W, x, w, b, dy)
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, b64, padding=1)
    y64.backward(dy.double())
    y64 = y64.detach()
    f32 = torch.float32
    assert torch.equal(y64.to(f32).double(), y64)
    return C1Case(geom, out_fp32, x.to(BF16), w, b, dy if out_fp32 else dy.to(BF16), y64.to(f32 if out_fp32 else BF16), x64.grad.to(BF16),
                  w64.grad.to(f32), b64.grad.to(f32), y64.to(f32))


Conv1x1Case = collections.namedtuple('Conv1x1Case', 'M cin cout x dy dw')


@functools.lru_cache(maxsize=None)
def conv1x1_case(M, Ci, Co):
    """dW (Cout, Cin) fp32 = dy^T x over M rows: x (M, Cin), dy (M, Cout) integer-valued bf16."""
    r = _ranges(('conv1x1', M, Ci, Co))
    g = torch.Generator().manual_seed(4000 + M + Ci + Co)
    x, dy = ints(g, (M, Ci), r['x']), ints(g, (M, Co), r['dy'])
    assert_sums_exact(f'conv1x1_wgrad M {M} {Ci}->{Co}', 0, 0, M, x, None, None, dy)
    dw = dy.double().t() @ x.double()
    return Conv1x1Case(M, Ci, Co, x.to(BF16), dy.to(BF16), dw.to(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------- comparison
def mismatches(got, ref, names, first=5):
    """(count, ['(n=.., channel=.., y=.., x=..): got .. expected ..', ...]) of the elements where ``got`` is not equal to ``ref`` (NaN-strict),
    in row-major order of the LOGICAL shape, so a failing tap, border row or channel piece can be read off."""
    bad = ~(got == ref)
    idx = bad.nonzero()
    lines = []
    for row in idx[:first].tolist():
        where = ', '.join(f'{n}={i}' for n, i in zip(names, row))
        lines.append(f'({where}): got {float(got[tuple(row)])!r} expected {float(ref[tuple(row)])!r}')
    return int(idx.shape[0]), lines


def assert_equal(got, ref, names, what):
    """Bit-for-bit: ``torch.equal`` on the CPU, in the dtype the kernel stores.  ``names``: one name per dimension (NCHW, OIRS, OI)."""
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape and len(names) == ref.dim(), (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    count, lines = mismatches(got, ref, names)
    raise AssertionError(f'{what}: {count} of {ref.numel()} elements differ from the exact reference; first: ' + '; '.join(lines))
