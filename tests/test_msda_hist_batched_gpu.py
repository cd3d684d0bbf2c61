"""The binning passes of the d_value record pipeline (msda_hist_raw_k: count and fill) take several sampling points per lane and trip.
These cases aim at the edges of that batching; d_value is compared with the CPU oracle, the record count with a count made on the CPU."""
import ctypes

import pytest
import torch

from oracle import gedepth_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = ((20, 37), (10, 19), (5, 10), (3, 5))       # no width a multiple of the tile's 8, no height a multiple of its 4
NH, L, P = 8, 4, 8
N_OFF = NH * L * P * 2
TW, TH = 8, 4                                        # value tile of a bin (csrc/msda.h)
BATCH = 1024 * 8                                     # sampling points a workgroup takes per trip: 1024 lanes x the larger U of the two passes

_CASES = {
    # name: (B, Nq) -> R query ranges per (image, head) = min(ceil(512 / (B * nH)), Nq // 64), a unit = one range of one (image, head)
    'ragged-batches': (2, 9605),     # R = 32, 300 or 301 queries = 9600 / 9632 points per unit: one full trip of 8192 and a tail that ends inside a 1024-point pass
    'short-unit': (1, 50),           # R = 1, 1600 points: less than one trip, passes 2 .. 7 of it have no live lane
    'uneven-ranges': (1, 777),       # R = 12, 64 or 65 queries per range
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def _pixels(raw, ref):
    """Sampling positions in pixel units (x, y) and the map sizes, float64, (B, Nq, nH, L, P) — mmcv's arithmetic on the bf16 offsets."""
    B, Nq, _ = raw.shape
    wh = torch.tensor([[w, h] for h, w in SHAPES], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
    pix = (ref.double()[:, :, None, :, None, :] + raw[..., :N_OFF].double().view(B, Nq, NH, L, P, 2) / wh) * wh - 0.5
    return pix[..., 0], pix[..., 1], wh[..., 0], wh[..., 1]


def _inputs(B, Nq, seed):
    """Random reference points over [-0.1, 1.1]^2 and offsets of a few pixels: points outside the maps, in their border cells and across tile
    edges.  A point within 2e-3 pixels of an integer coordinate is drawn again: there the last bit of the fp32 location decides the cell
    (the kernel's error is ~1e-4 pixels at these sizes), and the record count below is compared exactly."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.cat((torch.randn(B, Nq, N_OFF, generator=g) * 3.0, torch.randn(B, Nq, NH * L * P, generator=g)), -1).bfloat16()
    ref = (torch.rand(Nq, 2, generator=g) * 1.2 - 0.1)[None, :, None, :].expand(B, Nq, L, 2).contiguous()
    for _ in range(20):
        x, y, _, _ = _pixels(raw, ref)
        near = ((x - x.round()).abs() < 2e-3) | ((y - y.round()).abs() < 2e-3)
        if not bool(near.any()):
            break
        redraw = (torch.randn(B, Nq, NH, L, P, 2, generator=g) * 3.0).bfloat16()
        off = raw[..., :N_OFF].view(B, Nq, NH, L, P, 2)
        raw[..., :N_OFF] = torch.where(near[..., None], redraw, off).view(B, Nq, N_OFF)
    else:
        raise AssertionError('could not move every sampling point off the cell boundaries')
    value = torch.randn(B, sum(h * w for h, w in SHAPES), NH, 64, generator=g).bfloat16()
    go = torch.randn(B, Nq, NH * 64, generator=g).bfloat16()
    return value, raw, ref, go


def _tiles_per_point(raw, ref, level_mask):
    """Number of value tiles that hold an in-map bilinear corner of each sampling point (0 for a point outside or on a masked level)."""
    x, y, W, H = _pixels(raw, ref)
    on = torch.tensor([(level_mask >> l) & 1 for l in range(L)], dtype=torch.bool).view(1, 1, 1, L, 1)
    valid = (x > -1) & (y > -1) & (x < W) & (y < H) & on
    x0, y0 = x.floor(), y.floor()
    two_x = (x0 >= 0) & (x0 + 1 < W) & (((x0 + 1) / TW).floor() != (x0 / TW).floor())
    two_y = (y0 >= 0) & (y0 + 1 < H) & (((y0 + 1) / TH).floor() != (y0 / TH).floor())
    tiles = valid.long() * (1 + two_x.long()) * (1 + two_y.long())
    last_col, last_row = valid & (x0 == W - 1), valid & (y0 == H - 1)
    return tiles, last_col, last_row


@pytest.mark.parametrize('case,level_mask', [('ragged-batches', 15), ('ragged-batches', 6), ('short-unit', 15), ('uneven-ranges', 15), ('uneven-ranges', 9)])
def test_msda_hist_batched_records_vs_oracle(dev, case, level_mask, monkeypatch):
    """kernels._bwd_value_records (ge_msda_bwd_value_raw_levels) on shapes at the edges of the batched binning loop: d_value against the
    oracle's value gradient on the same bf16-rounded tensors at the bound of test_msda_bf16_gradients_vs_oracle (1e-2 of the tensor's
    scale), rows of masked levels untouched, and — exactly — the records the count pass counted against the (point, tile) pairs counted
    on the CPU."""
    from gedepth_amd import hip, kernels as K
    B, Nq = _CASES[case]
    value, raw, ref, go = _inputs(B, Nq, seed=100 + sum(map(ord, case)))
    Nv = value.shape[1]
    lv = K._levels(SHAPES)
    plan = (ctypes.c_int * 4)()
    hip.check(hip.lib().ge_msda_bwd_plan(lv.ptr, B, Nv, Nq, NH, L, P, plan), 'plan')
    assert plan[0] == 1
    R, nbins = plan[1], plan[3]
    per_unit = sorted({(Nq * (r + 1) // R - Nq * r // R) * L * P for r in range(R)})
    if case == 'ragged-batches':
        assert all(n > BATCH and n % BATCH and n % BATCH % 1024 for n in per_unit) and Nq % R, per_unit
    elif case == 'short-unit':
        assert R == 1 and per_unit[0] < BATCH and per_unit[0] % 1024, per_unit
    else:
        assert Nq % R and len(per_unit) == 2, per_unit
    tiles, last_col, last_row = _tiles_per_point(raw, ref, level_mask)
    assert set(tiles.unique().tolist()) == {0, 1, 2, 4}                 # outside / inside one tile / across an edge / across a corner
    assert bool(last_col.any()) and bool(last_row.any())                # right-hand / lower corners outside the map
    # oracle: mmcv's arithmetic in fp32 on the CPU, differentiated by autograd
    vc = value.float().requires_grad_(True)
    norm = torch.tensor([[w, h] for h, w in SHAPES], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref[:, :, None, :, None, :] + raw[..., :N_OFF].float().view(B, Nq, NH, L, P, 2) / norm
    aw = raw[..., N_OFF:].float().view(B, Nq, NH, L * P).softmax(-1).view(B, Nq, NH, L, P)
    O.msda_core(vc, SHAPES, loc, aw).backward(go.float())
    want = vc.grad.clone()
    start = 0
    for l, (h, w) in enumerate(SHAPES):
        if not (level_mask >> l) & 1:
            want[:, start:start + h * w] = 0
        start += h * w
    # the call's workspace is its own: keep a handle on it to read the bin counts back
    raw_d, go_d = raw.to(dev), go.to(dev)
    raw_ref, _ = K._raw_ref(raw_d, ref.to(dev), NH, L, P)
    d_value = torch.zeros(B, Nv, NH, 64, device=dev)
    real_empty, kept = K.torch.empty, []                               # the allocator the wrapper itself looks up (a guard harness may have replaced it)

    def keeping_empty(*a, **kw):
        t = real_empty(*a, **kw)
        if kw.get('dtype') is torch.uint8:
            kept.append(t)
        return t
    monkeypatch.setattr(K.torch, 'empty', keeping_empty)
    K._bwd_value_records(raw_d, raw_ref, go_d, d_value, lv, NH, L, P, level_mask)
    torch.cuda.synchronize()
    monkeypatch.setattr(K.torch, 'empty', real_empty)
    assert len(kept) == 1
    counted = int(kept[0][:nbins * 4].view(torch.int32).sum().item())   # MsdaWs.cnt is the first block of the workspace
    print(f'\n[msda hist {case} mask {level_mask:04b}] R {R} points per unit {per_unit} records {counted} (CPU {int(tiles.sum())})')
    assert counted == int(tiles.sum())
    scale = want.abs().max().item() + 1e-12
    err = (d_value.cpu().double() - want.double()).abs().max().item()
    print(f'[msda hist {case} mask {level_mask:04b}] d_value max abs err / scale {err / scale:.2e}')
    assert err <= 1e-2 * scale, f'd value: max abs err {err:.3e} vs scale {scale:.3e}'
