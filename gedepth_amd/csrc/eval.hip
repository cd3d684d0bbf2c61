// Metric sums of the KITTI evaluation protocol on the device (include/gedepth_eval.h; depth/core/evaluation.py `calculate` behind
// depth/datasets/kitti.py `pre_eval`): one image leaves the GPU as ten f64 numbers.  ge_depth_metrics_resized (include/gedepth_ddad.h) is the
// same reduction for the DDAD protocol, with the bilinear resize of the prediction to the ground truth folded into the pass.
//
// The discontinuous part is numpy's float32 arithmetic, bit for bit: gt = (float)raw / depth_scale, the mask gt > min && gt < max, and
// ratio = maximum(gt / pred, pred / gt) < 1.25^p with true IEEE divisions (no reciprocal, no contraction) and a NaN-propagating maximum.
// The six continuous terms are formed in f64 from the two f32 values and summed in f64: at 352 x 1216 the f64 rate does not matter, the
// pass streams 1.7 MB + 0.9 MB and is sized by launch latency.
//
// Reduction without atomics (the library is built with -munsafe-fp-atomics, and an atomic sum would depend on arrival order): a lane sums
// its groups of four pixels, a wave folds its lanes with shuffles, a workgroup folds its four waves through LDS and stores ten doubles to
// partials[block]; metrics_fold_k, one workgroup on the same stream, adds the partials in index order.  Same bits on every run.
#pragma clang fp contract(off)
#include "eval_sums.h"
#include "../../include/gedepth_eval.h"
#include "../../include/gedepth_ddad.h"

template <bool PV, bool GV>
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_partial_k(const float* __restrict__ pred, const uint16_t* __restrict__ gt_raw,
                                                                     EvalArgs a, double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  metrics_window_sums<PV, GV>(pred, gt_raw, a, acc);                  // eval_sums.h
  metrics_block_fold(acc, red, partials + (long)blockIdx.x * GE_EVAL_SUMS);
}

// DDAD protocol (depth/datasets/ddad.py pre_eval): the (h, w) prediction is resized bilinearly, align_corners = True, to the (H, W) ground
// truth, and every pixel with lo < gt < hi counts.  The kernel walks the ground truth in groups of four pixels; a group without a counted
// pixel loads nothing of the prediction (DDAD: ~1 % of 1216 x 1936 is valid), a counted pixel gathers its four taps and never stores the
// resized value.  Source index and weights are ge_scale(.., true) / ge_lerp(.., true) of common.h, whose align-corners branch computes exactly
// scale = (float)(h - 1) / (float)(H - 1) (0 when H == 1), src = scale * (float)Y, i0 = (int)src, i1 = min(i0 + 1, h - 1), w1 = src - (float)i0,
// w0 = 1.f - w1 (its clamp of i0 to h - 1 never acts: src < h); the blend is the expression of aug_resize_k, ATen's
// wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11), in f32 without contraction.
// GV: gt is 16-byte aligned and W % 4 == 0 (one float4 per group); otherwise element loads, each one bounds-checked against W.
struct ResizedArgs { int h, w, H, W; float lo, hi; };
template <bool GV>
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_resized_partial_k(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                             ResizedArgs a, double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  const float sy = ge_scale(a.h, a.H, true), sx = ge_scale(a.w, a.W, true);
  const int G = (a.W + 3) >> 2;                                       // groups per ground-truth row
  const long items = (long)a.H * G;
  for (long it = (long)blockIdx.x * GE_EVAL_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * GE_EVAL_THREADS) {
    const int r = (int)(it / G), c = 4 * (int)(it - (long)r * G);
    const float* gs = gt + (long)r * a.W + c;
    float g[4];
    if (GV) {
      const float4 t = *(const float4*)gs;
      g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = c + k < a.W ? gs[k] : 0.f;
    }
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) any = any || (c + k < a.W && g[k] > a.lo && g[k] < a.hi);
    if (!any) continue;                                               // no counted pixel in this group: no prediction loads
    const Lerp ly = ge_lerp(r, a.h, sy, true);
    const float* p0 = pred + (long)ly.i0 * a.w;
    const float* p1 = pred + (long)ly.i1 * a.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool inside = c + k < a.W;
      if (!(inside && g[k] > a.lo && g[k] < a.hi)) continue;
      const Lerp lx = ge_lerp(c + k, a.w, sx, true);
      const float v00 = p0[lx.i0], v01 = p0[lx.i1], v10 = p1[lx.i0], v11 = p1[lx.i1];
      const float p = ly.w0 * (lx.w0 * v00 + lx.w1 * v01) + ly.w1 * (lx.w0 * v10 + lx.w1 * v11);
      metric_pixel(p, g[k], inside, a.lo, a.hi, acc);
    }
  }
  metrics_block_fold(acc, red, partials + (long)blockIdx.x * GE_EVAL_SUMS);
}

__global__ void __launch_bounds__(GE_WAVE) metrics_fold_k(const double* __restrict__ partials, int blocks, double* __restrict__ sums) {
  if (threadIdx.x >= GE_EVAL_SUMS) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += partials[(long)b * GE_EVAL_SUMS + threadIdx.x];
  sums[threadIdx.x] = s;
}

extern "C" size_t ge_depth_metrics_workspace(int Hc, int Wc) {
  if (Hc <= 0 || Wc <= 0) return 0;
  return (size_t)metrics_blocks(Hc, Wc) * GE_EVAL_SUMS * sizeof(double);
}

extern "C" int ge_depth_metrics(const float* pred, const uint16_t* gt_raw, int H, int W, int top, int left, int Hc, int Wc,
                                int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth,
                                double* partials, double* sums, void* stream) {
  if (!pred || !gt_raw || !partials || !sums || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0) return GE_ERR_BAD_ARG;
  if (top < 0 || left < 0 || Hc > H - top || Wc > W - left) return GE_ERR_BAD_ARG;                  // the window lies in the frame
  if (r0 < 0 || r0 > Hc || r1 < 0 || r1 > Hc || c0 < 0 || c0 > Wc || c1 < 0 || c1 > Wc) return GE_ERR_BAD_ARG;
  if (((uintptr_t)pred & 3) || ((uintptr_t)gt_raw & 1) || ((uintptr_t)partials & 7) || ((uintptr_t)sums & 7)) return GE_ERR_UNSUPPORTED;
  hipStream_t s = ge_stream(stream);
  EvalArgs a;
  a.W = W; a.top = top; a.left = left; a.Hc = Hc; a.Wc = Wc; a.r0 = r0; a.r1 = r1; a.c0 = c0; a.c1 = c1;
  a.scale = depth_scale; a.lo = min_depth; a.hi = max_depth;
  const unsigned blocks = metrics_blocks(Hc, Wc);
  const bool pv = ((uintptr_t)pred & 15) == 0 && (Wc & 3) == 0;
  const bool gv = pv && ((uintptr_t)gt_raw & 7) == 0 && (W & 3) == 0 && (left & 3) == 0;
  if (gv)
    metrics_partial_k<true, true><<<blocks, GE_EVAL_THREADS, 0, s>>>(pred, gt_raw, a, partials);
  else if (pv)
    metrics_partial_k<true, false><<<blocks, GE_EVAL_THREADS, 0, s>>>(pred, gt_raw, a, partials);
  else
    metrics_partial_k<false, false><<<blocks, GE_EVAL_THREADS, 0, s>>>(pred, gt_raw, a, partials);
  GE_LAUNCH_CHECK();
  metrics_fold_k<<<1, GE_WAVE, 0, s>>>(partials, (int)blocks, sums);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" size_t ge_depth_metrics_resized_workspace(int H, int W) { return ge_depth_metrics_workspace(H, W); }

extern "C" int ge_depth_metrics_resized(const float* pred, int h, int w, const float* gt, int H, int W, float min_depth, float max_depth,
                                        double* partials, double* sums, void* stream) {
  if (!pred || !gt || !partials || !sums || h <= 0 || w <= 0 || H <= 0 || W <= 0) return GE_ERR_BAD_ARG;
  if (((uintptr_t)pred & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)sums & 7)) return GE_ERR_UNSUPPORTED;
  hipStream_t s = ge_stream(stream);
  ResizedArgs a;
  a.h = h; a.w = w; a.H = H; a.W = W; a.lo = min_depth; a.hi = max_depth;
  const unsigned blocks = metrics_blocks(H, W);
  if (((uintptr_t)gt & 15) == 0 && (W & 3) == 0)
    metrics_resized_partial_k<true><<<blocks, GE_EVAL_THREADS, 0, s>>>(pred, gt, a, partials);
  else
    metrics_resized_partial_k<false><<<blocks, GE_EVAL_THREADS, 0, s>>>(pred, gt, a, partials);
  GE_LAUNCH_CHECK();
  metrics_fold_k<<<1, GE_WAVE, 0, s>>>(partials, (int)blocks, sums);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
