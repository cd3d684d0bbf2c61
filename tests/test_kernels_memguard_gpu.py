"""Every launching entry point of gedepth_amd/kernels.py under red zones and poisoned buffers (tests/memguard.py).

The value tests compare results; they cannot see a kernel that writes past an output or a workspace, leaves part of an output unwritten, or
reads a buffer before writing it, because recycled allocator blocks are mapped and mostly zero.  Each case here re-runs the BODY of an existing
value test (imported from its module: the same inputs, reference and tolerances — this file adds no tolerance of its own), at the edge shapes,
while ``kernels.torch`` is the harness's proxy, once per poison byte.  So every output, gradient and workspace the wrappers allocate (forward and
backward) sits in a poisoned frame, tensors the test body allocates on the device or copies to it are framed too (``frame_copies_on``), and

1. no guard byte of any frame has changed (``Guard.check``);
2. the body's own comparisons hold (NaN-strict ``close``): a read of poison that reaches a result fails them;
3. no element of an ``empty`` allocation of kernels.py holds the poison pattern under BOTH poison bytes at the same position (never stored),
   except the allocations of ``PARTLY_WRITTEN`` (workspaces sized by an upper bound, each with its reason);
4. the entry points the case claims (``covers``) were really called.

The last test (no GPU needed) reads the entry-point names out of kernels.py and requires each to be covered by a case.
Not covered here: allocations made outside kernels.py by mmrt/optim.py beyond the one FusedAdamW case, depth/datasets/gpu_pipeline.py (the
``ge_aug_*`` kernels) and the inference / visualisation engines' own buffers."""
import ast
import collections
import os

import pytest
import torch

import memguard
import conv_exact
import test_conv1x1_bn_gpu as CB
import test_conv_exact_gpu as TX
import test_inference_gpu as TI
import test_kernels_gpu as TK
import test_msda_hist_batched_gpu as HB
import test_visualize_gpu as TV
import test_window_attn_gpu as TW
from test_visualize_cpu import CASES as COLORIZE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS_PY = os.path.join(ROOT, 'gedepth_amd', 'kernels.py')

Case = collections.namedtuple('Case', 'name covers run')
Ctx = collections.namedtuple('Ctx', 'dev monkeypatch golden')

TINY = ((3, 5), (2, 3), (1, 2), (1, 1))                                    # the 'tiny' geometry of TK._MM_CASES, for the streaming kernels
SMALL = ((11, 35), (6, 18), (3, 9), (2, 5))

WIN = {'ge_window_attn_fwd', 'ge_window_attn_bwd'}
MSDA = {'ge_msda_fwd', 'ge_msda_bwd'}
MM = {'ge_msda_fwd_mm', 'ge_msda_bwd_lw_mm', 'ge_msda_dref', 'ge_msda_bwd_value_mm', 'ge_msda_bwd_value_raw_levels', 'ge_msda_bwd_value_vs'}
LN = {'ge_layernorm_fwd', 'ge_layernorm_bwd_multi', 'ge_layernorm_fold'}


def _each(fn, *param_lists):
    """run(ctx) that calls ``fn(ctx, *params)`` for every combination."""
    def run(ctx):
        import itertools
        for params in itertools.product(*param_lists):
            fn(ctx, *params)
    return run


def _colorize(ctx):
    by_name = {c[0]: c for c in COLORIZE_CASES}
    for name in ('python-bounds', 'none-none-finite'):            # given bounds; the data's min / max (the partial-reduction workspace)
        TV.test_colorize_bit_exact(*by_name[name])


CASES = [
    # ---- window attention: variants 1 (fp32) and 2 (bf16 MFMA) in one body, variant 3 (fp8 forward); maps smaller / larger than a window
    Case('window_attn v1+v2 (3,5) nH3', WIN, _each(lambda c, s: TK.test_window_attention_mfma_vs_exact(c.dev, (2, 3, 5, 3), s), (0, 3))),
    Case('window_attn v1+v2 (7,7) nH24', WIN, _each(lambda c, s: TK.test_window_attention_mfma_vs_exact(c.dev, (3, 7, 7, 24), s), (0, 3))),
    Case('window_attn v1+v2 (10,9) (11,35)', WIN, _each(lambda c, g, s: TK.test_window_attention_mfma_vs_exact(c.dev, g, s),
                                                        ((2, 10, 9, 3), (2, 11, 35, 3)), (0, 3))),
    Case('window_attn module fp32 vs oracle', WIN, _each(lambda c, hw, s: TK.test_window_attention_fp32_fwd_bwd(c.dev, hw, s),
                                                         ((3, 5), (10, 9), (11, 35)), (0, 3))),
    Case('window_attn v3 fp8', WIN, _each(lambda c, gs: TK.test_window_attention_fp8_forward(c.dev, *gs),
                                          (((2, 11, 35, 3), 0), ((2, 11, 35, 3), 3), ((2, 10, 9, 6), 0)))),
    # routed inputs, bit for bit, where the last window row and column hold one real row / column (variants 1, 2, 3); 243 windows over 64 persistent
    # workgroups per head (test_window_attn_gpu.py)
    Case('window_attn routed (8,15) nH6 shift 3', WIN, lambda c: TW.test_routing_bit_for_bit(c.dev, (1, 8, 15, 6), 3)),
    Case('window_attn many windows per workgroup', WIN, lambda c: TW.test_many_windows_per_workgroup(c.dev)),
    # ---- deformable attention: streaming and query-grid kernels, every kernel-selection mode, binned / atomic backward
    Case('msda streaming fp32 small+tiny', MSDA, _each(lambda c, b, sh: TK.test_msda_fp32_fwd_bwd(c.dev, b, sh, c.monkeypatch), (True, False), (SMALL, TINY))),
    Case('msda window kernels ragged f32', MSDA, lambda c: TK.test_msda_window_kernels(c.dev, 'ragged', 'f32')),        # modes 7 3 0 8 13 61 125 29
    Case('msda window kernels ragged bf16', MSDA, lambda c: TK.test_msda_window_kernels(c.dev, 'ragged', 'bf16')),
    Case('msda bf16 modes binned', MSDA, _each(lambda c, m: TK.test_msda_bf16_gradients_vs_oracle(c.dev, m, True, c.monkeypatch), (0, 7, 8, 13, 29, 61, 125))),
    Case('msda bf16 modes atomic', MSDA, _each(lambda c, m: TK.test_msda_bf16_gradients_vs_oracle(c.dev, m, False, c.monkeypatch), (0, 7, 8, 13, 29, 61, 125))),
    Case('msda many records per tile', MSDA, _each(lambda c, m: TK.test_msda_drain_many_records_per_tile(c.dev, m), (125, 61, 29, 13))),
    Case('msda per-head histograms', MSDA, lambda c: TK.test_msda_large_maps_use_per_head_histograms(c.dev)),
    Case('msda_prepare', {'ge_msda_prep_fwd', 'ge_msda_prep_bwd'},
         _each(lambda c, P, dt: TK.test_msda_prepare_matches_mmcv_arithmetic(c.dev, P, dt), (8, 4), ('f32', 'bf16'))),
    Case('msda raw f32', {'ge_msda_fwd_raw', 'ge_msda_bwd_raw'} | MSDA | {'ge_msda_prep_fwd', 'ge_msda_prep_bwd'},
         _each(lambda c, k: TK.test_msda_raw_fused_prepare_and_sampling(c.dev, 'f32', k), ('self', 'cross'))),
    Case('msda raw bf16', {'ge_msda_fwd_raw', 'ge_msda_bwd_raw', 'ge_msda_bwd_value_raw_levels'},
         _each(lambda c, k: TK.test_msda_raw_fused_prepare_and_sampling(c.dev, 'bf16', k), ('self', 'cross'))),
    Case('msda mm ragged', MM, lambda c: TK.test_msda_mm_fwd_bwd_vs_oracle(c.dev, 'ragged')),          # GE_MSDA_VALUE records, mm, 12, 5, 10, vs inside
    Case('msda mm tiny', MM, lambda c: TK.test_msda_mm_fwd_bwd_vs_oracle(c.dev, 'tiny')),
    Case('msda mm strays', MM, lambda c: TK.test_msda_mm_fwd_bwd_vs_oracle(c.dev, 'strays')),
    Case('msda mm scattered', MM, lambda c: TK.test_msda_mm_fwd_bwd_vs_oracle(c.dev, 'scattered')),
    Case('msda self split odd sizes', {'ge_msda_fwd_mm_part', 'ge_msda_bwd_lw_mm_part', 'ge_msda_fwd_raw', 'ge_msda_bwd_raw', 'ge_msda_bwd_value_raw_levels'},
         lambda c: TK.test_msda_self_split_vs_oracle_and_window_kernels(c.dev, ((37, 53), (19, 27), (10, 14), (5, 7)))),
    Case('msda batched count/fill', {'ge_msda_bwd_value_raw_levels'},
         _each(lambda c, k: HB.test_msda_hist_batched_records_vs_oracle(c.dev, k[0], k[1], c.monkeypatch),
               (('ragged-batches', 15), ('ragged-batches', 6), ('short-unit', 15), ('uneven-ranges', 15), ('uneven-ranges', 9)))),
    # ---- convolutions
    Case('conv3x3 v1', {'ge_conv3x3_nhwc_fwd', 'ge_conv3x3_nhwc_wgrad', 'ge_bias_act_nhwc_bwd', 'ge_colsum'},
         _each(lambda c, g, a: TK.test_conv3x3_mfma_vs_conv2d(c.dev, g, a, '1', c.monkeypatch), ((2, 32, 32, 3, 5), (1, 160, 64, 13, 37), (2, 96, 96, 9, 33)), (False, True))),
    Case('conv3x3 v2', {'ge_conv3x3_nhwc_fwd', 'ge_conv3x3_nhwc_wgrad', 'ge_bias_act_nhwc_bwd', 'ge_colsum'},
         _each(lambda c, g, a: TK.test_conv3x3_mfma_vs_conv2d(c.dev, g, a, '2', c.monkeypatch), ((2, 32, 32, 3, 5), (1, 160, 64, 13, 37), (2, 96, 96, 9, 33)), (False, True))),
    Case('conv3x3_c1', {'ge_conv3x3_c1_fwd', 'ge_conv3x3_c1_bwd'},
         _each(lambda c, g, f: TK.test_conv3x3_one_output_channel_vs_conv2d(c.dev, g, f), ((3, 128, 1, 1), (1, 72, 9, 5), (2, 64, 13, 37)), (False, True))),
    Case('conv1x1_bn_act_pos', {'ge_conv1x1_bn_stats', 'ge_conv1x1_bn_act_fwd', 'ge_conv1x1_bn_bwd_mask', 'ge_conv1x1_nhwc_wgrad', 'ge_conv1x1_bn_bwd_finalize',
                                'ge_conv1x1_bn_dgrad'},
         _each(lambda c, k: TK.test_conv1x1_bn_act_pos_vs_fp32_composition(c.dev, *k),
               (((1, 64, 33, 17), 512, 'tokens'), ((3, 64, 7, 9), 256, 'both'), ((2, 64, 24, 40), 512, 'slice')))),
    # rows < 32, HW < 32, no position map, one row; Cout = 1024 (the widest Wd, one dgrad workgroup per CU) and 384 (odd chunk count, idle act_k waves)
    Case('conv1x1_bn_act_pos edges', {'ge_conv1x1_bn_stats', 'ge_conv1x1_bn_act_fwd', 'ge_conv1x1_bn_bwd_mask', 'ge_conv1x1_nhwc_wgrad',
                                      'ge_conv1x1_bn_bwd_finalize', 'ge_conv1x1_bn_dgrad'},
         lambda c: ([CB.test_tile_and_channel_edges(c.dev, c.monkeypatch, *k) for k in
                     (((1, 64, 3, 5), 128, True), ((3, 64, 1, 31), 128, True), ((3, 64, 3, 11), 128, False), ((2, 64, 7, 9), 384, True),
                      ((2, 64, 7, 9), 1024, True))], CB.test_one_row(c.dev))),
    Case('conv1x1 as token GEMM', set(), lambda c: TK.test_conv1x1_as_token_gemm_vs_fp32_conv(c.dev, (2, 96, 24, 40), 512)),
    Case('conv1x1_wgrad', {'ge_conv1x1_nhwc_wgrad'}, lambda c: TK.test_conv1x1_wgrad_vs_float64(c.dev, (1, 64, 544, 30, 33), c.monkeypatch)),
    # ---- the convolution kernels bit for bit on integer data (test_conv_exact_gpu.py): the prefetching, persistent and split-K loops past their
    # first tile / unit / stage, and a Cout that is a multiple of 8 only
    Case('conv3x3 exact v1', {'ge_conv3x3_nhwc_fwd', 'ge_conv3x3_nhwc_wgrad', 'ge_bias_act_nhwc_bwd'},
         lambda c: TX.test_conv3x3_exact(c.dev, (2, 96, 96, 9, 33), 0.5, '1', c.monkeypatch)),
    Case('conv3x3 exact v2', {'ge_conv3x3_nhwc_fwd', 'ge_conv3x3_nhwc_wgrad', 'ge_bias_act_nhwc_bwd'},
         lambda c: TX.test_conv3x3_exact(c.dev, (2, 96, 96, 17, 33), 0.0, '2', c.monkeypatch)),
    Case('conv3x3 exact C ABI Cout 40', {'ge_conv3x3_nhwc_fwd', 'ge_conv3x3_nhwc_wgrad'},
         _each(lambda c, v: TX.test_conv3x3_c_abi_partial_cout(c.dev, 40, v, c.monkeypatch), ('1', '2'))),
    Case('conv3x3_wgrad exact several tiles per workgroup', {'ge_conv3x3_nhwc_wgrad'},
         lambda c: TX.test_conv3x3_wgrad_several_tiles_per_workgroup(c.dev, 0.5)),
    Case('conv3x3_c1 exact several units per workgroup', {'ge_conv3x3_c1_fwd', 'ge_conv3x3_c1_bwd'},
         _each(lambda c, f: TX.test_conv3x3_c1_exact(c.dev, conv_exact.C1_MULTI_UNIT_BWD, 'bwd-walks', f), (False, True))),
    Case('conv1x1_wgrad exact several stages per workgroup', {'ge_conv1x1_nhwc_wgrad'},
         lambda c: TX.test_conv1x1_wgrad_exact(c.dev, 192, 544, 'stages', c.monkeypatch)),
    # ---- token GEMM and its epilogues
    Case('gemm_nt', {'ge_gemm_nt'}, _each(lambda c, s, b: TK.test_gemm_nt_vs_float64(c.dev, s, b), ((255, 8, 8), (257, 72, 8), (513, 136, 520), (1000, 520, 264)), (True, False))),
    Case('bias_gelu', {'ge_bias_gelu_fwd', 'ge_bias_gelu_bwd'},
         _each(lambda c, dt, rc: TK.test_bias_gelu_epilogue(c.dev, dt, *rc), ('f32', 'bf16'), ((5, 8), (777, 384), (1001, 3072)))),
    Case('colsum', {'ge_colsum'}, _each(lambda c, k: TK.test_colsum_vs_float64(c.dev, *k), ((777, 100, 'f32'), (5, 8, 'bf16'), (33, 4104, 'bf16'), (1001, 2304, 'bf16')))),
    # ---- normalisation, residuals
    Case('layer_norm', LN, _each(lambda c, C, io: TK.test_layer_norm_mixed_precision(c.dev, C, io), (100, 3072), ('f32->f32', 'f32->bf16', 'bf16->bf16', 'bf16->f32'))),
    Case('layer_norm_res', LN, _each(lambda c, d: TK.test_layer_norm_with_skip_gradient(c.dev, d), ('f32->bf16', 'bf16->bf16', 'f32->f32'))),
    Case('residual_drop_path', {'ge_residual_scale_add', 'ge_scale_rows'},
         _each(lambda c, d, s: TK.test_residual_drop_path(c.dev, d, s), ('f32+f32', 'f32+bf16', 'bf16+bf16'), ((4, 37, 96), (3, 5, 7)))),
    Case('residual_dropout add_rows', {'ge_concat_rows_fwd', 'ge_slice_rows_drop', 'ge_add_rows'}, lambda c: TK.test_residual_dropout_and_add_rows(c.dev)),
    Case('bn_act nchw', {'ge_bn_act_fwd', 'ge_bn_act_bwd'}, _each(lambda c, s, d: TK.test_bn_act_training(c.dev, (2, 5, 7, 9), s, d), (0.0, 1.0), ('f32', 'bf16'))),
    Case('bias_act nchw', {'ge_bias_act_fwd', 'ge_bias_act_bwd'}, _each(lambda c, sh, s: TK.test_bias_act_fp32(c.dev, sh, s), ((2, 5, 7, 9), (1, 3, 1, 1)), (1.0, 0.0, 0.01))),
    Case('nhwc bn_act bias_act bilinear', {'ge_bn_act_nhwc_fwd', 'ge_bn_act_nhwc_bwd', 'ge_bias_act_nhwc_fwd', 'ge_bias_act_nhwc_bwd', 'ge_bilinear_nhwc_fwd',
                                           'ge_bilinear_nhwc_bwd'},
         _each(lambda c, d, g: TK.test_nhwc_bn_act_bias_act_bilinear_match_nchw(c.dev, d, g), ('f32', 'bf16'), ((3, 96, 7, 9), (2, 8, 33, 17)))),
    # ---- resampling and decoder glue
    Case('bilinear nchw', {'ge_bilinear_fwd', 'ge_bilinear_bwd'},
         _each(lambda c, a, s: TK.test_bilinear_fwd_bwd(c.dev, a, s), (False, True), (((1, 2), (8, 12)), ((16, 31), (7, 9)), ((7, 9), (16, 31))))),
    Case('upcat', {'ge_upcat_nhwc_fwd', 'ge_upcat_nhwc_bwd'},
         _each(lambda c, d, g: TK.test_upcat_matches_interpolate_cat(c.dev, d, g), ('f32', 'bf16'), ((2, 16, 24, (1, 2), (2, 3)), (2, 8, 8, (5, 7), (9, 13))))),
    Case('upsum', {'ge_upsum_nhwc_fwd', 'ge_bilinear_nhwc_bwd'}, _each(lambda c, d: TK.test_upsum_matches_pe_trunk_composition(c.dev, d), ('f32', 'bf16'))),
    Case('tokens_from_map concat_tokens_map', {'ge_tokens_from_map', 'ge_map_from_tokens'},
         _each(lambda c, g, d: TK.test_tokens_from_map_and_back(c.dev, g, d), ((1, 7, 3, 5), (3, 72, 9, 8)), ('f32', 'bf16'))),
    Case('concat_tokens_map slice + dropout', {'ge_tokens_from_map', 'ge_map_from_tokens'}, lambda c: TK.test_concat_tokens_map_token_slice_and_dropout(c.dev)),
    Case('nhwc token glue', {'ge_concat_rows_fwd', 'ge_slice_rows_drop', 'ge_add_rows'},
         _each(lambda c, d, f: TK.test_nhwc_token_map_glue_matches_nchw(c.dev, d, f), ('f32', 'bf16'), (True, False))),
    # ---- ground embedding, fusion, loss, offline maps, inference, visualisation
    Case('ground_embed_adaptive (33,47)', {'ge_ground_embed_fwd', 'ge_ground_embed_bwd'}, _each(lambda c, h: TK.test_ground_embed_adaptive(c.dev, (33, 47), h), (False, True))),
    Case('ground_embed_vanilla', {'ge_ground_vanilla_fwd', 'ge_ground_vanilla_bwd'}, lambda c: TK.test_ground_embed_vanilla_bwd(c.dev)),
    Case('depth_fuse', {'ge_depth_fuse_fwd', 'ge_depth_fuse_bwd'}, lambda c: TK.test_depth_fuse(c.dev)),
    Case('silog_loss', {'ge_silog_stats', 'ge_silog_bwd'}, lambda c: TK.test_silog(c.dev, c.golden)),
    Case('ground_plane slope_class pe_channels', {'ge_ground_plane', 'ge_slope_class', 'ge_pe_channels'}, lambda c: TK.test_ground_plane_and_slope_class_bit_exact(c.dev)),
    Case('slope_class_ddad', {'ge_ground_plane', 'ge_slope_class', 'ge_slope_class_ddad'}, lambda c: TK.test_ground_plane_and_slope_classes_vs_reference_scripts(c.dev, c.golden)),
    Case('infer_front', {'ge_infer_front'}, lambda c: TI.test_front_end_equals_training_pipeline_chain()),
    Case('tta_merge', {'ge_tta_merge'}, lambda c: TI.test_tta_merge_bit_exact()),
    Case('depth_colorize', {'ge_depth_colorize'}, _colorize),
    # ---- the optimizer's flat arena (gedepth_amd/mmrt/optim.py allocates in its own module: the same proxy, installed there too)
    Case('fused_adamw arena', set(), lambda c: TK.test_fused_adamw_matches_torch(c.dev)),
]

# Allocations of kernels.py that are only partly written BY DESIGN, by the variable they are assigned to: workspaces whose size function is an upper
# bound over what one call touches, and staging tensors.  Everything else that comes from torch.empty / empty_like must be stored in full.
PARTLY_WRITTEN = {
    'ws': 'kernel workspaces: sized by ge_*_workspace() for the worst case (record chunks, per-workgroup partials); a call touches the part its geometry needs',
    'mm_ws': 'ge_msda_bwd_mm_workspace / ge_msda_bwd_vs_workspace: tap boxes and run lists for the maximum number of tiles and runs',
    'host': "_MMValueChoice.observe: the framed CPU tensor is only the source of pin_memory()'s copy; the pinned copy is what copy_ fills",
    'scratch': 'ground / fuse backward scratch planes: partial sums of the rows a workgroup owns, sized for the full map',
}

EXEMPT = {
    'ge_msda_bwd_timing_read': 'reads the host-side per-stage timing totals of ge_msda_bwd into host variables: no launch, no device memory',
}

_FIRST = {}                    # case name -> (poison, {allocation key: flat indices that held the poison pattern}) of the run that came first


def _assigned_name(frame):
    text = frame.site[2]
    head = text.split('=')[0].strip() if '=' in text else ''
    return head.split(',')[0].strip()


def _poison_positions(frames):
    """{(site line, shape, dtype, occurrence): CPU indices of the interior elements that hold the poison pattern} over the ``empty`` allocations
    of kernels.py that must be written in full."""
    out, seen = {}, collections.Counter()
    for f in frames:
        if f.kind != 'empty' or os.path.abspath(f.site[0]) != KERNELS_PY or not f.raw.is_cuda or f.nbytes == 0:
            continue
        key = (f.site[1], f.shape, str(f.dtype))
        seen[key] += 1
        if _assigned_name(f) in PARTLY_WRITTEN:
            continue
        out[key + (seen[key],)] = (f.poisoned().nonzero().flatten().cpu(), f.describe())
    return out


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()
    return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name.replace(' ', '_'))
def test_guarded(dev, monkeypatch, golden, case, poison):
    from gedepth_amd import hip, kernels
    from gedepth_amd.mmrt import optim
    guard = memguard.Guard(poison)
    # cached per-stream workspaces / accumulators made by earlier (unguarded) tests would bypass the frames
    for cache in ('_LN_ACC', '_COLSUM_WS', '_POS_ROWS', '_TILE_ORDER_CACHE', '_MM_VALUE_CHOICE'):
        monkeypatch.setattr(kernels, cache, {})
    guard.install(monkeypatch, [kernels, optim, TK, TI, HB, CB, TX, TW], binding=hip, frame_copies_on=dev)
    failure = None
    try:
        case.run(Ctx(dev, monkeypatch, golden))           # 2. the value test's own comparisons, NaN-strict
        torch.cuda.synchronize()
    except Exception as e:                                # look at the red zones first: an overrun explains a wrong value, not the other way round
        failure = e
    monkeypatch.undo()                                    # the harness's own checks below run on the real torch
    try:
        frames = guard.check()                            # 1. red zones (raises with call site, side and offsets)
    except AssertionError as e:
        raise e from failure
    called = set(guard.launched) | set(guard.direct)
    positions = _poison_positions(frames)
    first = _FIRST.get(case.name)
    never = []
    if first is None or first[0] == poison:
        _FIRST[case.name] = (poison, {k: v for k, v in positions.items() if v[0].numel()})
        print(f'\n[memguard {case.name} {poison:#04x}] {len(frames)} frames, {len(positions)} outputs checked; the never-written check needs the '
              f'run with the other poison byte, which has not run: skipped here, done by that run')
    else:                                                 # 3. never-written elements: poison pattern under both bytes at the same position
        for key, (idx, what) in positions.items():
            other = first[1].get(key)
            if other is not None and idx.numel():
                both = idx[torch.isin(idx, other[0])]
                if both.numel():
                    never.append(f'{what}: {both.numel()} elements never written, flat index {int(both[0])} .. {int(both[-1])}')
        print(f'\n[memguard {case.name}] {len(frames)} frames, {len(positions)} outputs checked under both poison bytes')
    if never:                                             # reported even when the value comparison failed too: it says why
        raise AssertionError('unwritten output elements:\n  ' + '\n  '.join(never[:12])) from failure
    if failure is not None:
        raise failure
    assert case.covers <= called, f'{case.name}: claimed but not called: {sorted(case.covers - called)}'          # 4.


def _entry_points_of_kernels_py():
    with open(KERNELS_PY) as fh:
        tree = ast.parse(fh.read())
    names, forwarded = set(), 0
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Name) and f.id == '_launch':
            arg = node.args[2]
        elif isinstance(f, ast.Attribute) and f.attr == 'call' and isinstance(f.value, ast.Name) and f.value.id == 'hip':
            arg = node.args[0]
        else:
            continue
        if isinstance(arg, ast.Name):                     # _launch itself forwards its ``name`` parameter to hip.call (twice: profiled or not)
            forwarded += 1
            continue
        assert isinstance(arg, ast.Constant) and isinstance(arg.value, str) and arg.value.startswith('ge_'), ast.dump(arg)
        names.add(arg.value)
    assert forwarded == 2, 'an entry-point name that is not a literal: this test cannot see what it launches'
    return names


def test_every_entry_point_of_kernels_py_is_covered_by_a_case():
    from gedepth_amd import hip
    names = _entry_points_of_kernels_py()
    assert len(names) >= 70, len(names)
    covered = set().union(*(c.covers for c in CASES))
    assert not (covered & set(EXEMPT)), sorted(covered & set(EXEMPT))
    assert all(n in hip.SIGNATURES for n in EXEMPT) and all(n in hip.SIGNATURES for n in covered)
    missing = names - covered - set(EXEMPT)
    assert not missing, f'entry points of kernels.py that no guarded case covers: {sorted(missing)}'
    assert len({c.name for c in CASES}) == len(CASES)
