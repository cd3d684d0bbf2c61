"""Float64 reference of the shifted-window attention core (what ``gedepth_amd.kernels.window_attention`` computes between the qkv and proj
Linears), written from the definition: pad to multiples of 7 (pad tokens carry the qkv bias), roll by -shift, partition, nine-region mask as an
ADDITIVE -100, relative-position bias, softmax, PV, reverse, roll back, crop.  No GPU, no kernel code, none of the oracle's helpers.

``core``           float64, differentiable with autograd: the reference the kernels are compared with.
``tables``         per window, the 49 source-token indices (-1: pad) and the mask-region ids.
``model``          the same computation in the kernels' arithmetic on the CPU, backward written out by hand; it only SETS TOLERANCES: its error
                   against ``core`` is what the number formats alone cost.
``routed_inputs``  inputs on which the attention is an exact gather in every arithmetic (one-hot softmax), for bit-for-bit tests.
"""
import torch

WS, WT, HD, NBIAS = 7, 49, 32, 169


def _windows(grid):
    """(Hp, Wp) -> (nW, 49): 7x7 windows in row-major window order, row-major inside a window."""
    Hp, Wp = grid.shape
    return grid.view(Hp // WS, WS, Wp // WS, WS).permute(0, 2, 1, 3).reshape(-1, WT)


def tables(H, W, shift):
    """tok (nW, 49): index of the source token in the un-padded (H, W) grid, -1 for a pad token; reg (nW, 49): region id of the shift mask."""
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    src = torch.full((Hp, Wp), -1, dtype=torch.long)
    src[:H, :W] = torch.arange(H * W).view(H, W)
    reg = torch.zeros(Hp, Wp, dtype=torch.long)
    if shift > 0:
        src = torch.roll(src, shifts=(-shift, -shift), dims=(0, 1))
        cnt = 0
        for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):        # regions live on the padded, rolled grid
            for ws_ in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
                reg[hs, ws_] = cnt
                cnt += 1
    return _windows(src), _windows(reg)


def rel_index():
    """(49, 49): entry of the 13x13 bias table for (query, key) = (iq - ik + 6) * 13 + (jq - jk + 6)."""
    i, j = torch.arange(WT) // WS, torch.arange(WT) % WS
    return (i[:, None] - i[None, :] + 6) * 13 + (j[:, None] - j[None, :] + 6)


def _geometry(H, W, shift):
    tok, reg = tables(H, W, shift)
    L = H * W
    flat = tok.reshape(-1)
    real = (flat >= 0).nonzero().flatten()
    inv = torch.empty(L, dtype=torch.long)
    inv[flat[real]] = real                                    # token -> its (window, position) slot
    pad = (flat < 0).nonzero().flatten()
    mask = None
    if shift > 0:
        mask = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0)     # (nW, query, key)
    return tok, flat, inv, pad, mask


def columns(nH, heads):
    heads = list(range(nH)) if heads is None else list(heads)
    c = torch.cat([torch.arange(h * HD, (h + 1) * HD) for h in heads])
    C = nH * HD
    return heads, torch.cat([c, C + c, 2 * C + c])


def _gather(x, padrow, flat):
    """x (B, L, ch), padrow (ch,) -> (B, nW*49, ch): pad slots take padrow."""
    B, L, ch = x.shape
    xp = torch.cat([x, padrow.view(1, 1, ch).expand(B, 1, ch)], 1)
    return xp[:, torch.where(flat >= 0, flat, torch.full_like(flat, L))]


def core(qkv, qkv_bias, table, H, W, nH, shift, scale, heads=None):
    """qkv (B, H*W, 3*nH*32), qkv_bias (3*nH*32,), table (169, nH) -> (B, H*W, len(heads)*32) in float64.  ``heads`` (default: all) restricts the
    work to a subset of heads; gradients of the other heads' inputs are then zero."""
    f64 = torch.float64
    B, L, _ = qkv.shape
    assert L == H * W and qkv.shape[2] == 3 * nH * HD
    heads, cols = columns(nH, heads)
    nh = len(heads)
    table = table.to(f64)
    tok, flat, inv, _, mask = _geometry(H, W, shift)
    nW = tok.shape[0]
    win = _gather(qkv[:, :, cols].to(f64), qkv_bias[cols].to(f64), flat).view(B, nW, WT, 3, nh, HD).permute(3, 0, 1, 4, 2, 5)
    q, k, v = win[0], win[1], win[2]                                           # (B, nW, nh, 49, 32)
    s = (q * scale) @ k.transpose(-1, -2)
    s = s + table[:, heads][rel_index().reshape(-1)].view(WT, WT, nh).permute(2, 0, 1)
    if mask is not None:
        s = s + mask.to(f64)[None, :, None]
    o = s.softmax(-1) @ v
    o = o.permute(0, 1, 3, 2, 4).reshape(B, nW * WT, nh * HD)
    return o[:, inv]


def _bf16(x):
    return x.bfloat16().to(x.dtype)


def model(qkv, qkv_bias, table, go, H, W, nH, shift, scale, arith, heads=None):
    """Forward and hand-written backward in the kernels' arithmetic.  Returns out (B, L, nh*32), d_qkv (B, L, 3*nh*32: q | k | v of the chosen
    heads), d_qkv_bias (3*nh*32), d_table (169, nh).

    arith 'f32':  float32 throughout (the exact-fp32 kernel);  'f64': float64 throughout (to check this backward against autograd of ``core``);
    'bf16': float32 with the roundings to bf16 that the MFMA kernels make: the pad value; P before PV; P and dS before the key-side (dV, dK)
    and query-side (dQ) products; out and d_qkv on store.  delta, dS itself, the table gradient and the pad-token bias gradient stay float32.
    Inputs are expected storage-rounded already."""
    dt = torch.float64 if arith == 'f64' else torch.float32
    r = _bf16 if arith == 'bf16' else (lambda x: x)
    qkv, qkv_bias, table, go = qkv.to(dt), qkv_bias.to(dt), table.to(dt), go.to(dt)
    B, L, _ = qkv.shape
    heads, cols = columns(nH, heads)
    nh = len(heads)
    tok, flat, inv, pad, mask = _geometry(H, W, shift)
    nW = tok.shape[0]
    win = _gather(qkv[:, :, cols], r(qkv_bias[cols]), flat).view(B, nW, WT, 3, nh, HD).permute(3, 0, 1, 4, 2, 5)
    q, k, v = win[0], win[1], win[2]
    rel = rel_index().reshape(-1)
    s = (q @ k.transpose(-1, -2)) * scale + table[:, heads][rel].view(WT, WT, nh).permute(2, 0, 1)
    if mask is not None:
        s = s + mask.to(dt)[None, :, None]
    p = s.softmax(-1)
    o = r(r(p) @ v).permute(0, 1, 3, 2, 4).reshape(B, nW * WT, nh * HD)
    out = o[:, inv]
    # backward: dP = dO V^T, delta = sum_k P dP, dS = P (dP - delta)
    gcols = cols[:nh * HD]
    g = _gather(go[:, :, gcols], torch.zeros(nh * HD, dtype=dt), flat).view(B, nW, WT, nh, HD).permute(0, 1, 3, 2, 4)
    dp = g @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    d_table = torch.zeros(NBIAS, nh, dtype=dt).index_add_(0, rel, ds.sum((0, 1)).reshape(nh, WT * WT).t())
    dq = (r(ds) @ k) * scale
    dk = (r(ds).transpose(-1, -2) @ q) * scale
    dv = r(p).transpose(-1, -2) @ g
    dwin = torch.stack([dq, dk, dv]).permute(1, 2, 4, 0, 3, 5).reshape(B, nW * WT, 3 * nh * HD)
    d_qkv = r(dwin[:, inv])
    d_qkv_bias = dwin[:, pad].sum((0, 1))
    d_qkv_bias[:nh * HD] = 0                                  # pad queries get no output gradient
    return out, d_qkv, d_qkv_bias, d_table


def hadamard_codes():
    """(64, 32): the rows of the 32x32 Sylvester Hadamard matrix, then their negatives.  code[a] . code[b] = 32 if a == b, else 0 or -32."""
    h = torch.ones(1, 1)
    while h.shape[0] < HD:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return torch.cat([h, -h], 0).double()


def routed_inputs(B, H, W, nH, shift, seed, amplitude, cross_region=False):
    """Inputs on which every query attends to exactly one key.  The key at window position a is amplitude * code[a]; the query at a is
    amplitude * code[pi(a)], pi drawn per (batch, head, window): a permutation of the real tokens inside each mask region, or with
    ``cross_region`` a map of every real token to a real token of ANOTHER region (windows whose real tokens share one region keep a
    permutation).  v and the v part of qkv_bias hold integers in [-7, 7], one element of every token's head slice is 7; the q and k parts of
    qkv_bias are 0.  All values are bf16-exact.

    Returns a dict: qkv, qkv_bias, go (bf16-exact N(0,1)), out = the expected gather v[pi(i)], dv = the inverse gather of go (None when some pi is
    no permutation), n_cross = how many queries point into another region."""
    g = torch.Generator().manual_seed(seed)
    C, L = nH * HD, H * W
    code = hadamard_codes()
    tok, reg = tables(H, W, shift)
    nW = tok.shape[0]
    v = torch.randint(-7, 8, (B, L, nH, HD), generator=g).double()
    v.scatter_(3, torch.randint(0, HD, (B, L, nH, 1), generator=g), 7.0)
    q, k = torch.zeros(B, L, nH, HD, dtype=torch.float64), torch.zeros(B, L, nH, HD, dtype=torch.float64)
    qkv_bias = torch.zeros(3 * C, dtype=torch.float64)
    qkv_bias[2 * C:] = torch.randint(-7, 8, (C,), generator=g).double()
    go = torch.randn(B, L, C, generator=g).bfloat16().double()
    out = torch.zeros(B, L, nH, HD, dtype=torch.float64)
    dv = torch.zeros(B, L, nH, HD, dtype=torch.float64)
    gov = go.view(B, L, nH, HD)
    n_cross, permutation = 0, True
    for w in range(nW):
        real = (tok[w] >= 0).nonzero().flatten()
        regions = reg[w][real].unique().tolist()
        for b in range(B):
            for h in range(nH):
                pi = torch.empty(WT, dtype=torch.long)
                if cross_region and len(regions) > 1:
                    for a in real.tolist():
                        other = real[reg[w][real] != reg[w][a]]
                        pi[a] = other[torch.randint(0, len(other), (1,), generator=g)]
                    n_cross += len(real)
                    permutation = False
                else:
                    for rg in regions:
                        pos = real[reg[w][real] == rg]
                        pi[pos] = pos[torch.randperm(len(pos), generator=g)]
                src, dst = tok[w][real], tok[w][pi[real]]
                k[b, src, h] = amplitude * code[real]
                q[b, src, h] = amplitude * code[pi[real]]
                out[b, src, h] = v[b, dst, h]
                dv[b, dst, h] = gov[b, src, h]
    qkv = torch.cat([q.view(B, L, C), k.view(B, L, C), v.view(B, L, C)], 2)
    return dict(qkv=qkv, qkv_bias=qkv_bias, go=go, out=out.view(B, L, C), dv=dv.view(B, L, C) if permutation else None, n_cross=n_cross)


def errors(a, ref):
    """(l2rel, max-abs error over the reference's maximum) of ``a`` against the float64 ``ref``; both 0 when they agree and ref is all zero."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = a - ref
    if not bool(torch.isfinite(d).all()):
        return float('inf'), float('inf')
    n, m = ref.norm().item(), ref.abs().max().item()
    dn, dm = d.norm().item(), d.abs().max().item()
    return (dn / n if n > 0 else (0.0 if dn == 0 else float('inf'))), (dm / m if m > 0 else (0.0 if dm == 0 else float('inf')))
