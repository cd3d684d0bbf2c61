"""The exact-arithmetic method of tests/conv_exact.py, checked without a GPU: the generator honours the 2^24 bound and really exercises bf16
rounding, the float64 references are exact in fp32 too, and the comparison helper fails — naming the right element — for the subtle errors
that tests/test_conv_exact_gpu.py exists to catch: one dropped product, a truncation instead of a rounding, two swapped channels."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as X

CUS = 256                        # MI355X; only sizes the conv1x1 row counts here (the GPU test recomputes them from the device)

CONV3X3_ALL = tuple((g, s) for g in X.CONV3X3_GEOMS + (X.CONV3X3_WGRAD_MULTI_TILE, X.CONV3X3_WGRAD_AUTOGRAD) for s in X.SLOPES)
C1_ALL = tuple((g, f) for g in X.C1_GEOMS + (X.C1_MULTI_UNIT_BWD, X.C1_MULTI_UNIT_FWD) for f in (False, True))
CONV1X1_ALL = tuple((M, ci, co) for ci in X.CONV1X1_CIN for co in X.CONV1X1_COUT for M in X.conv1x1_rows(ci, co, CUS))


def _ids(v):
    return 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('geom,slope', CONV3X3_ALL, ids=_ids)
def test_conv3x3_cases_are_exact_and_exercise_rounding(geom, slope):
    """Every conv3x3 case: small integers, the sum of |products| per output below 2^24 (asserted by the builder), the reference equal to the
    same convolution evaluated in fp32 on the CPU, and — for Cin >= 96 — at least 1 % of y and of dx not representable in bf16 with at least
    one exact tie in each (the builder asserts it; the figures are repeated here)."""
    N, Ci, Co, H, W = geom
    c = X.conv3x3_case(geom, slope)
    assert all(v < X.LIMIT for v in c.bounds.values()), c.bounds
    assert c.bounds['issue'] == 9 * max(Ci, Co) * max(float(c.x.abs().max()), float(c.dy.abs().max())) * float(c.w.abs().max()) + float(c.b.abs().max())
    if Ci >= 96:
        for name in ('y', 'dx'):
            share, ties = c.rounding[name]
            assert share >= 0.01 and ties >= 1, (name, share, ties)
        assert not torch.equal(X.truncate_to_bf16(c.y32), c.y) and not torch.equal(X.truncate_to_bf16(c.dx32), c.dx)
    else:
        assert c.rounding is None and float(c.y32.abs().max()) <= 9 * Ci * 12 + 8
    # the same convolution in fp32: integers are exact there too, whatever order the CPU library sums in
    x, w, b = c.x.float().requires_grad_(True), c.w.clone().requires_grad_(True), c.b.clone().requires_grad_(True)
    y = X._act(F.conv2d(x, w, b, padding=1), slope)
    y.backward(c.dy.float())
    assert torch.equal(y.detach(), c.y32) and torch.equal(x.grad, c.dx32) and torch.equal(w.grad, c.dw) and torch.equal(b.grad, c.db)
    assert torch.equal(c.y32.to(X.BF16), c.y) and torch.equal(c.dx32.to(X.BF16), c.dx)
    # the masked gradient is what the backward of the convolution receives: dW from it, without the activation, is the same dW
    w2 = c.w.double().requires_grad_(True)
    F.conv2d(c.x.double(), w2, None, padding=1).backward(c.dyp.double())
    assert torch.equal(w2.grad.float(), c.dw)


@pytest.mark.parametrize('cout', X.CONV3X3_ABI_COUTS)
def test_conv3x3_abi_cases_are_exact(cout):
    c = X.conv3x3_abi_case(cout)
    y = X._act(F.conv2d(c.x.float(), c.w.float(), c.b, padding=1), c.slope)
    assert cout % 8 == 0 and cout % 32 != 0 and torch.equal(y.to(X.BF16), c.y)


@pytest.mark.parametrize('geom,out_fp32', C1_ALL, ids=_ids)
def test_conv3x3_c1_cases_are_exact(geom, out_fp32):
    c = X.c1_case(geom, out_fp32)
    x, w, b = c.x.float().requires_grad_(True), c.w.clone().requires_grad_(True), c.b.clone().requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    y.backward(c.dy.float())
    assert torch.equal(y.detach(), c.y32) and torch.equal(x.grad.to(X.BF16), c.dx) and torch.equal(w.grad, c.dw) and torch.equal(b.grad, c.db)
    assert float(x.grad.abs().max()) < 256                      # nine products per element: dx is exact in bf16, only y is rounded
    assert c.y.dtype == (torch.float32 if out_fp32 else X.BF16) and c.dy.dtype == c.y.dtype


def test_conv3x3_c1_multi_unit_shapes_exceed_the_grid_caps():
    assert X.c1_units(*[X.C1_MULTI_UNIT_BWD[i] for i in (0, 2, 3)]) == 1040 > X.C1_CAP_BWD
    assert X.c1_units(*[X.C1_MULTI_UNIT_FWD[i] for i in (0, 2, 3)]) == 4160 > X.C1_CAP_FWD
    assert all(X.c1_units(g[0], g[2], g[3]) <= 10 for g in X.C1_GEOMS)             # the basic shapes: at most one unit per workgroup


@pytest.mark.parametrize('M,ci,co', CONV1X1_ALL, ids=str)
def test_conv1x1_cases_are_exact(M, ci, co):
    c = X.conv1x1_case(M, ci, co)
    assert torch.equal(c.dy.float().t() @ c.x.float(), c.dw)
    stages, ksplit = X.conv1x1_wgrad_split(M, ci, co, CUS)
    if M != 2048 + 5:
        assert stages // ksplit >= 3 and M % X.CONV1X1_STAGE == 37 and stages % ksplit == 1


def test_split_rules_at_256_cus():
    tiles, ksplit = X.conv3x3_wgrad_split(X.CONV3X3_WGRAD_MULTI_TILE, CUS)
    assert (tiles, ksplit) == (56, 16) and tiles // ksplit >= 3 and tiles % ksplit != 0
    N, _, _, H, W = X.CONV3X3_WGRAD_AUTOGRAD
    assert N * H * W >= 10000


# ------------------------------------------------------------------------------------------- the comparison helper must be able to fail
def _first_index(mask):
    return tuple(mask.nonzero()[0].tolist())


def _where(names, idx):
    return '(' + ', '.join(f'{n}={i}' for n, i in zip(names, idx)) + ')'


@pytest.mark.parametrize('geom,slope', [((2, 96, 96, 9, 33), None), ((1, 160, 64, 13, 37), None)], ids=_ids)
def test_one_dropped_product_fails_and_is_located(geom, slope):
    """One single product (one (tap, ci) of one output pixel) removed from the reference: the fp32 value differs, and so does the bf16 value at
    every pixel below 256 (integers there are exact in bf16).  The message names the pixel and the channel."""
    c = X.conv3x3_case(geom, slope)
    N, Ci, Co, H, W = geom
    n, co, y, x, r, s, ci = N - 1, Co - 1, H - 1, W - 2, 0, 2, Ci - 1                 # last row: tap row 0 is inside the image, tap row 2 is not
    assert 0 <= y + r - 1 < H and 0 <= x + s - 1 < W
    # a nonzero product at a pixel whose value bf16 holds exactly
    prod = float(c.w[co, ci, r, s]) * float(c.x[n, ci, y + r - 1, x + s - 1])
    while prod == 0.0 or abs(float(c.y32[n, co, y, x])) >= 256 or abs(float(c.y32[n, co, y, x]) - prod) >= 256:
        ci -= 1
        if ci < 0:
            ci, x = Ci - 1, x - 1
        prod = float(c.w[co, ci, r, s]) * float(c.x[n, ci, y + r - 1, x + s - 1])
    wrong32 = c.y32.clone()
    wrong32[n, co, y, x] -= prod
    where = _where(X.NCHW, (n, co, y, x))
    for got, ref in ((wrong32, c.y32), (wrong32.to(X.BF16), c.y)):
        with pytest.raises(AssertionError) as e:
            X.assert_equal(got, ref, X.NCHW, 'y')
        assert '1 of ' in str(e.value) and where in str(e.value), str(e.value)
        assert f'got {float(got[n, co, y, x])!r} expected {float(ref[n, co, y, x])!r}' in str(e.value)
    # the weight gradient: one pixel's product dropped from one (co, ci, r, s)
    wrong = c.dw.clone()
    wrong[co, ci, r, s] -= float(c.dyp[n, co, y, x]) * float(c.x[n, ci, y + r - 1, x + s - 1]) or 1.0
    with pytest.raises(AssertionError) as e:
        X.assert_equal(wrong, c.dw, X.OIRS, 'dw')
    assert _where(X.OIRS, (co, ci, r, s)) in str(e.value)
    X.assert_equal(c.y.clone(), c.y, X.NCHW, 'y')                                    # and equal tensors pass


@pytest.mark.parametrize('geom,slope', [((2, 96, 96, 9, 33), None), ((2, 96, 96, 17, 33), 0.5), ((1, 160, 64, 13, 37), 0.0)], ids=_ids)
def test_truncation_instead_of_rounding_fails_and_is_located(geom, slope):
    c = X.conv3x3_case(geom, slope)
    for ref32, ref, what in ((c.y32, c.y, 'y'), (c.dx32, c.dx, 'dx')):
        low = ref32.contiguous().view(torch.int32) & 0xFFFF
        odd = (ref32.contiguous().view(torch.int32) >> 16) & 1
        rounds_up = (low > 0x8000) | ((low == 0x8000) & (odd == 1))                  # round-to-nearest-even goes away from the truncated value
        assert bool(rounds_up.any())
        got = X.truncate_to_bf16(ref32)
        with pytest.raises(AssertionError) as e:
            X.assert_equal(got, ref, X.NCHW, what)
        assert f'{int(rounds_up.sum())} of ' in str(e.value) and 'first: ' + _where(X.NCHW, _first_index(rounds_up)) in str(e.value), str(e.value)


def test_swapped_channels_fail_and_are_located():
    c = X.conv3x3_case((2, 32, 64, 2, 31), 0.5)
    a, b = 9, 40
    got = c.y.clone()
    got[:, a], got[:, b] = c.y[:, b], c.y[:, a]
    differ = torch.zeros_like(c.y, dtype=torch.bool)
    differ[:, a] = differ[:, b] = c.y[:, a] != c.y[:, b]
    with pytest.raises(AssertionError) as e:
        X.assert_equal(got, c.y, X.NCHW, 'y')
    first = _first_index(differ)
    assert first[1] == a and f'{int(differ.sum())} of ' in str(e.value) and 'first: ' + _where(X.NCHW, first) in str(e.value), str(e.value)
    # NaN never compares equal: an output that was not written (NaN poison) fails too
    got = c.dw.clone()
    got[3, 5, 1, 2] = float('nan')
    with pytest.raises(AssertionError, match=r'\(co=3, ci=5, r=1, s=2\)'):
        X.assert_equal(got, c.dw, X.OIRS, 'dw')
