"""The backward algebra of csrc/conv1x1_bn.hip restated in torch (no GPU): why its constant term c0 carries a compensation.

The fused 1x1 conv + training BatchNorm + ReLU block never stores the pre-BN tensor; its data gradient is

    dX = g A1 + X A2 + c0        A1 = diag(a) W,  A2 = - W^T diag(rstd a m2) W,  c0 = ((mean rstd m2 - m1) a)^T W

(file header of csrc/conv1x1_bn.hip), with [A1 | A2] stored in bf16 for the MFMAs and c0 in fp32.  ``X A2 + c0`` is the BatchNorm backward's
``- zhat * mean(g zhat)`` term written on the RAW input: with x = m + (x - m) the part ``m A2`` is a constant vector that c0 largely cancels.
Rounding A2 to bf16 leaves ``m (A2 - bf16(A2))`` uncancelled, an error that grows with the channel means m of the input, and that only shows
when d_gamma is not ~0, i.e. when the output gradient has a component along the normalised activation (it always has in training; plain
randn gradients do not).  conv1x1_bn_bwd_a2_k therefore adds ``m (A2_fp32 - bf16(A2_fp32))`` to c0.

This file restates that algebra with float64 contractions and bf16 roundings exactly where the kernels round (x, w, dy, g, A1, A2 and the stored dx), checks the
restatement against float64 autograd, and pins the finding: the uncompensated form degrades with the input offset, the compensated one does not.
"""
import pytest
import torch
import torch.nn.functional as F

ROWS, CIN, COUT, EPS = 4096, 64, 128, 1e-5
OFFSETS = (0, 4, 16)


def bf(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def l2rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def operands(r, correlated, seed=11):
    """x (rows, 64), w (Cout, 64), gamma, beta in float64 holding bf16 values (gamma / beta fp32 values), dy (rows, Cout) bf16 values."""
    g = torch.Generator().manual_seed(seed)
    sign = (torch.randint(0, 2, (CIN,), generator=g) * 2 - 1).double()
    x = bf(torch.randn(ROWS, CIN, generator=g).double() + r * sign)
    w = bf(torch.randn(COUT, CIN, generator=g).double() * 0.2)
    gamma = (torch.rand(COUT, generator=g) + 0.5).double()
    beta = (torch.randn(COUT, generator=g) * 0.3).double()
    dy = torch.randn(ROWS, COUT, generator=g).double()
    if correlated:
        z = x @ w.t()
        zhat = (z - z.mean(0)) / (z.var(0, unbiased=False) + EPS).sqrt()
        dy = dy + 0.7 + zhat
    return x, w, gamma, beta, bf(dy)


def autograd(x, w, gamma, beta, dy):
    x, w, gamma, beta = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
    y = F.relu(F.batch_norm(x @ w.t(), None, None, gamma, beta, True, 0.1, EPS))          # a 1x1 convolution is a matrix product over the rows
    y.backward(dy)
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad)


def kernel_algebra(x, w, gamma, beta, dy, a2, rounded=True):
    """The file header's formulas.  ``a2``: 'exact' (A2 kept in float64), 'bf16' (rounded, c0 as in the header: the form before the
    compensation), 'compensated' (rounded, residue times the channel means folded into c0).  ``rounded=False``: no rounding of g / A1 either."""
    rnd = bf if rounded else (lambda t: t)
    n = x.shape[0]
    s, S = x.sum(0), x.t() @ x                                   # column sums and Gram matrix of the input (conv1x1_gram_k)
    mean = (w @ s) / n                                            # conv1x1_bn_finalize_k: the statistics of z = x W^T from the input's moments
    var = ((w @ S) * w).sum(1) / n - mean * mean
    rstd = 1.0 / (var.clamp_min(0) + EPS).sqrt()
    a = gamma * rstd
    y = F.relu((x @ w.t()) * a + (beta - mean * a))
    g = rnd(dy * (y > 0))                                         # conv1x1_bn_mask_k: bf16, its column sums are those of the rounded values
    m1 = g.sum(0)
    G = g.t() @ x                                                 # ge_conv1x1_nhwc_wgrad, fp32 accumulation
    dgamma = rstd * (w * (G - m1[:, None] * s[None] / n)).sum(1)
    m1n, m2n = m1 / n, dgamma / n
    u = rstd[:, None] * (w @ S - mean[:, None] * s[None])
    dw = a[:, None] * (G - s[None] * m1n[:, None] - u * m2n[:, None])
    A1 = rnd(a[:, None] * w)
    k2, k0 = rstd * a * m2n, (mean * rstd * m2n - m1n) * a
    A2 = -(w.t() * k2) @ w
    c0 = k0 @ w
    if a2 != 'exact' and rounded:
        A2r = bf(A2)
        if a2 == 'compensated':
            c0 = c0 + (s / n) @ (A2 - A2r)
        A2 = A2r
    return dict(y=y, dx=rnd(g @ A1 + x @ A2 + c0), dw=dw, dgamma=dgamma, dbeta=m1)


@pytest.fixture(scope='module')
def dx_errors():
    """{(r, correlated, form): l2-relative error of dX against float64 autograd on the same bf16 operands}"""
    out = {}
    for r in OFFSETS:
        for correlated in (True, False):
            ops = operands(r, correlated)
            ref = autograd(*ops)['dx']
            for form in ('exact', 'bf16', 'compensated'):
                out[r, correlated, form] = l2rel(kernel_algebra(*ops, form)['dx'], ref)
    for k, v in out.items():
        print(f'[conv1x1_bn algebra] r={k[0]:>2} correlated={k[1]!s:5} {k[2]:11} dx l2rel {v:.2e}')
    return out


@pytest.mark.parametrize('r', OFFSETS)
def test_unrounded_algebra_is_the_batchnorm_backward(r):
    ops = operands(r, True)
    ref, got = autograd(*ops), kernel_algebra(*ops, 'exact', rounded=False)
    for k in ('y', 'dx', 'dw', 'dgamma', 'dbeta'):
        # float64 with the cancellation E[z^2] - mean^2 at |mean| / std up to ~16 * 8: 1e-9 leaves four digits of room
        assert l2rel(got[k], ref[k]) <= 1e-9, (k, l2rel(got[k], ref[k]))


@pytest.mark.parametrize('r', OFFSETS)
def test_parameter_gradients_do_not_depend_on_the_rounding_of_a2(r):
    ops = operands(r, True)
    ref, got = autograd(*ops), kernel_algebra(*ops, 'bf16')
    for k in ('dw', 'dgamma', 'dbeta'):
        assert l2rel(got[k], ref[k]) <= 6e-3, (k, l2rel(got[k], ref[k]))       # the bf16 storage of g, the GPU tests' bound


def test_bf16_a2_error_grows_with_the_input_offset_under_correlated_gradients(dx_errors):
    assert dx_errors[16, True, 'bf16'] > 3 * dx_errors[0, True, 'bf16'], dx_errors
    # ... and plain randn gradients (d_gamma ~ 0) do not show it: why the first kernel test of this block could not
    assert dx_errors[16, False, 'bf16'] <= 1.3 * dx_errors[0, False, 'bf16'], dx_errors


@pytest.mark.parametrize('r', OFFSETS)
def test_compensated_c0_keeps_dx_at_the_exact_a2_level(dx_errors, r):
    assert dx_errors[r, True, 'compensated'] <= 1.3 * dx_errors[r, True, 'exact'], dx_errors
