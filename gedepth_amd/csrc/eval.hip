// Metric sums of the KITTI evaluation protocol on the device (include/gedepth_eval.h; depth/core/evaluation.py `calculate` behind
// depth/datasets/kitti.py `pre_eval`): one image leaves the GPU as ten f64 numbers.  ge_depth_metrics_resized (include/gedepth_ddad.h) is the
// same reduction for the DDAD protocol, with the bilinear resize of the prediction to the ground truth folded into the pass;
// ge_depth_metrics_resized_batch (include/gedepth_ddad_batch.h) runs it for up to GE_BATCH_MAX images of one ground-truth size.
//
// The discontinuous part is numpy's float32 arithmetic, bit for bit: gt = (float)raw / depth_scale, the mask gt > min && gt < max, and
// ratio = maximum(gt / pred, pred / gt) < 1.25^p with true IEEE divisions (no reciprocal, no contraction) and a NaN-propagating maximum.
// The six continuous terms are formed in f64 from the two f32 values and summed in f64: at 352 x 1216 the f64 rate does not matter, the
// pass streams 1.7 MB + 0.9 MB and is sized by launch latency.
//
// Reduction without atomics (the library is built with -munsafe-fp-atomics, and an atomic sum would depend on arrival order): a lane sums
// its groups of four pixels, a wave folds its lanes with shuffles, a workgroup folds its four waves through LDS and stores ten doubles to
// partials[block]; metrics_fold_k, one workgroup per image on the same stream, adds the partials in index order.  Same bits on every run.
// The KITTI kernels take up to GE_BATCH_MAX images per launch (ge_depth_metrics_batch, include/gedepth_batch.h), the image on blockIdx.y
// of the first pass and blockIdx.x of the fold; ge_depth_metrics is their launch of one image.  ge_depth_metrics_strata[_batch]
// (include/gedepth_strata.h) is the same walk once per stratum of the ground truth, the stratum on blockIdx.z.
#pragma clang fp contract(off)
#include "batch_table.h"
#include "../../include/gedepth_eval.h"
#include "../../include/gedepth_ddad.h"
#include "../../include/gedepth_ddad_batch.h"
#include "../../include/gedepth_strata.h"
#include <cmath>

#define GE_EVAL_THREADS 256
#define GE_EVAL_GROUPS 2           // groups of four pixels per lane before the grid-stride loop goes round again
#define GE_EVAL_MAX_BLOCKS 1024
#define GE_EVAL_SUMS 10

struct EvalArgs { int Hc, Wc, r0, r1, c0, c1; float scale, lo, hi; };     // the crop, the protocol's rectangle in it, gt = raw / scale, lo < gt < hi

// One pixel: `gt` in metres (f32), `inside` = it lies in the protocol's rectangle; it counts when also lo < gt < hi.
__device__ __forceinline__ void metric_pixel(float p, float gt, bool inside, float lo, float hi, double acc[GE_EVAL_SUMS]) {
  if (!(inside && gt > lo && gt < hi)) return;
  const float q0 = gt / p, q1 = p / gt;
  const float ratio = (q0 > q1 || q0 != q0) ? q0 : q1;               // numpy.maximum: NaN wins
  acc[0] += 1.0;
  acc[1] += ratio < 1.25f ? 1.0 : 0.0;
  acc[2] += ratio < 1.5625f ? 1.0 : 0.0;
  acc[3] += ratio < 1.953125f ? 1.0 : 0.0;
  const double g = (double)gt, q = (double)p;
  const double d = g - q, d2 = d * d;
  const double l = log(q) - log(g);
  acc[4] += fabs(d) / g;
  acc[5] += d2 / g;
  acc[6] += d2;
  acc[7] += l;
  acc[8] += l * l;
  acc[9] += fabs(log10(g) - log10(q));
}

// lane sums -> wave (shuffles) -> workgroup (LDS across the four waves) -> partials[block]
// `row`: the ten doubles of this workgroup in the partials
__device__ __forceinline__ void metrics_block_fold(double acc[GE_EVAL_SUMS], double (*red)[GE_EVAL_SUMS], double* __restrict__ row) {
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k)
    for (int s = GE_WAVE / 2; s > 0; s >>= 1) acc[k] += __shfl_down(acc[k], s, GE_WAVE);
  const int wave = threadIdx.x / GE_WAVE, lane = threadIdx.x % GE_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < GE_EVAL_SUMS; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < GE_EVAL_SUMS) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < GE_EVAL_THREADS / GE_WAVE; ++w) s += red[w][threadIdx.x];
    row[threadIdx.x] = s;
  }
}

// Which pixels of a group count, beyond the rectangle and lo < gt < hi.  EveryPixel: all of them (ge_depth_metrics).
struct EveryPixel {
  static constexpr bool kSelects = false;
  __device__ __forceinline__ void group(int, int, const float*, bool*) const {}
};

// The pixels of ONE stratum (include/gedepth_strata.h): stratum = bin * C + on_ground, bin = #{ j : gt >= e[j] },
// on_ground = g > 0 && |gt - g| <= tol * g in f32 without contraction.  `ground` (row stride W) starts at the crop's corner, null: C = 1.
// gvec: a group's four ground depths are one 16-byte load (only with PV; W % 4 == 0, left % 4 == 0, base 16-byte aligned).
struct StratumArgs { float e[GE_STRATA_MAX_EDGES]; int n_edges, C; float tol; };
struct OneStratum {
  static constexpr bool kSelects = true;
  StratumArgs a;
  const float* __restrict__ ground;
  int W, s;
  bool gvec;
  // take[k]: pixel k of the group at (r, c) counts so far, gt[k] its ground truth; clears the ones outside stratum s
  __device__ __forceinline__ void group(int r, int c, const float gt[4], bool take[4]) const {
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (ground) {
      const float* gs = ground + (long)r * W + c;
      if (gvec) {
        if (take[0] || take[1] || take[2] || take[3]) {
          const float4 t = *(const float4*)gs;
          g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (take[k]) g[k] = gs[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int bin = 0;
#pragma unroll
      for (int j = 0; j < GE_STRATA_MAX_EDGES; ++j) bin += (j < a.n_edges && gt[k] >= a.e[j]) ? 1 : 0;
      const bool on = g[k] > 0.f && fabsf(gt[k] - g[k]) <= a.tol * g[k];        // a NaN g compares false: off the ground
      take[k] = take[k] && bin * a.C + (on ? 1 : 0) == s;
    }
  }
};

// One lane's sums over the crop of one image, as workgroup blockIdx.x of gridDim.x.  `gt_raw` (row stride W) starts at the crop's corner.
// PV: pred is 16-byte aligned and Wc % 4 == 0 (one float4 per group).  GV (only with PV): every group's four ground-truth values are
// 8-byte aligned (W % 4 == 0, left % 4 == 0, base 8-byte aligned).  Otherwise element loads, each one bounds-checked against Wc.
// Sel picks among the counted pixels (EveryPixel, OneStratum); a selecting walk loads pred only for a group with a pixel left.  A pixel
// that does not count adds nothing, so the lane's sums are those of EveryPixel on a ground truth that is 0 outside the selection.
template <bool PV, bool GV, class Sel>
__device__ __forceinline__ void metrics_window_sums(const float* __restrict__ pred, const uint16_t* __restrict__ gt_raw, int W, const EvalArgs& a,
                                                    const Sel& sel, double acc[GE_EVAL_SUMS]) {
  const int G = (a.Wc + 3) >> 2;                                      // groups per row
  const long items = (long)a.Hc * G;
  for (long it = (long)blockIdx.x * GE_EVAL_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * GE_EVAL_THREADS) {
    const int r = (int)(it / G), c = 4 * (int)(it - (long)r * G);
    if (r < a.r0 || r >= a.r1 || c + 4 <= a.c0 || c >= a.c1) continue;        // nothing of this group is in the rectangle: no loads
    const float* ps = pred + (long)r * a.Wc + c;
    const uint16_t* gs = gt_raw + (long)r * W + c;
    float p[4];
    uint16_t raw[4];
    auto load_pred = [&]() {
      if (PV) {
        const float4 t = *(const float4*)ps;
        p[0] = t.x; p[1] = t.y; p[2] = t.z; p[3] = t.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = c + k < a.Wc ? ps[k] : 1.f;
      }
    };
    if (!Sel::kSelects) load_pred();
    if (PV && GV) {
      const uint2 t = *(const uint2*)gs;
      raw[0] = (uint16_t)t.x; raw[1] = (uint16_t)(t.x >> 16); raw[2] = (uint16_t)t.y; raw[3] = (uint16_t)(t.y >> 16);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) raw[k] = c + k < a.Wc ? gs[k] : (uint16_t)0;
    }
    float gt[4];
    bool take[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                                 // gt = (float)raw / depth_scale; c1 <= Wc covers the row's tail
      gt[k] = (float)raw[k] / a.scale;
      take[k] = c + k >= a.c0 && c + k < a.c1;
    }
    if (Sel::kSelects) {
#pragma unroll
      for (int k = 0; k < 4; ++k) take[k] = take[k] && gt[k] > a.lo && gt[k] < a.hi;
      sel.group(r, c, gt, take);
      if (!(take[0] || take[1] || take[2] || take[3])) continue;                  // no pixel of this selection in the group: no prediction loads
      load_pred();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) metric_pixel(p[k], gt[k], take[k], a.lo, a.hi, acc);
  }
}

// the block partition of one image: it depends on (Hc, Wc) only
static unsigned metrics_blocks(int Hc, int Wc) {
  return ge_blocks((long)Hc * ((Wc + 3) >> 2), GE_EVAL_THREADS * GE_EVAL_GROUPS, GE_EVAL_MAX_BLOCKS);
}

// Image f = blockIdx.y of the table (batch_table.h; `image` the (H, W) uint16 ground truth): pred (n, Hc, Wc), partials (n, gridDim.x, 10).
// The ground truth's 8-byte loads (GV) are a per-image choice, uniform over the workgroup.  The images share the block partition, so an
// image's bits do not depend on how many images the launch has: ge_depth_metrics is the launch of one.
template <bool PV>
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_partial_k(const float* __restrict__ pred, BatchTable t, EvalArgs a,
                                                                     double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  const GeBatchFrame fr = t.f[blockIdx.y];
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  const float* p = pred + (long)blockIdx.y * a.Hc * a.Wc;
  const uint16_t* gt = (const uint16_t*)fr.image + ((long)fr.top * fr.W + fr.left);
  if (PV && ((uintptr_t)fr.image & 7) == 0 && (fr.W & 3) == 0 && (fr.left & 3) == 0)
    metrics_window_sums<PV, true>(p, gt, fr.W, a, EveryPixel(), acc);
  else
    metrics_window_sums<PV, false>(p, gt, fr.W, a, EveryPixel(), acc);
  metrics_block_fold(acc, red, partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * GE_EVAL_SUMS);
}

// Stratified sums (include/gedepth_strata.h): stratum s = blockIdx.z of image f = blockIdx.y walks the crop as metrics_partial_k does and
// adds the pixels of s only; partials (n, S, gridDim.x, 10).  fr.aux: the frame's (H, W) f32 ground depth, or null.  The crop is read S
// times (from L2 after the first), the logarithms are taken once per counted pixel in total.  No per-lane accumulators indexed by stratum.
template <bool PV>
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_strata_partial_k(const float* __restrict__ pred, BatchTable t, EvalArgs a, StratumArgs sa,
                                                                            double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  const GeBatchFrame fr = t.f[blockIdx.y];
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  const float* p = pred + (long)blockIdx.y * a.Hc * a.Wc;
  const long corner = (long)fr.top * fr.W + fr.left;
  const uint16_t* gt = (const uint16_t*)fr.image + corner;
  const bool aligned = PV && (fr.W & 3) == 0 && (fr.left & 3) == 0;
  OneStratum sel;
  sel.a = sa;
  sel.ground = fr.aux ? (const float*)fr.aux + corner : nullptr;
  sel.W = fr.W;
  sel.s = (int)blockIdx.z;
  sel.gvec = aligned && ((uintptr_t)fr.aux & 15) == 0;
  if (aligned && ((uintptr_t)fr.image & 7) == 0)
    metrics_window_sums<PV, true>(p, gt, fr.W, a, sel, acc);
  else
    metrics_window_sums<PV, false>(p, gt, fr.W, a, sel, acc);
  metrics_block_fold(acc, red, partials + (((long)blockIdx.y * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x) * GE_EVAL_SUMS);
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
// one lane's sums over the ground truth of one image, as workgroup blockIdx.x of gridDim.x
template <bool GV>
__device__ __forceinline__ void metrics_resized_sums(const float* __restrict__ pred, const float* __restrict__ gt, const ResizedArgs& a,
                                                     double acc[GE_EVAL_SUMS]) {
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
}

// Image f = blockIdx.y of the table (batch_table.h; `image` the (H, W) f32 ground truth, one size for all images): pred (n, h, w), partials
// (n, gridDim.x, 10).  The ground truth's 16-byte loads (GV) are a per-image choice, uniform over the workgroup.  The images share the block
// partition, so an image's bits do not depend on how many images the launch has: ge_depth_metrics_resized is the launch of one
// (include/gedepth_ddad_batch.h).
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_resized_partial_k(const float* __restrict__ pred, BatchTable t, ResizedArgs a,
                                                                             double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  const GeBatchFrame fr = t.f[blockIdx.y];
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  const float* p = pred + (long)blockIdx.y * a.h * a.w;
  const float* gt = (const float*)fr.image;
  if (((uintptr_t)fr.image & 15) == 0 && (a.W & 3) == 0)
    metrics_resized_sums<true>(p, gt, a, acc);
  else
    metrics_resized_sums<false>(p, gt, a, acc);
  metrics_block_fold(acc, red, partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * GE_EVAL_SUMS);
}

// row blockIdx.x (an image, or an (image, stratum) pair): its partials in index order
__global__ void __launch_bounds__(GE_WAVE) metrics_fold_k(const double* __restrict__ partials, int blocks, double* __restrict__ sums) {
  if (threadIdx.x >= GE_EVAL_SUMS) return;
  const double* p = partials + (long)blockIdx.x * blocks * GE_EVAL_SUMS;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += p[(long)b * GE_EVAL_SUMS + threadIdx.x];
  sums[(long)blockIdx.x * GE_EVAL_SUMS + threadIdx.x] = s;
}

extern "C" size_t ge_depth_metrics_batch_workspace(int n, int Hc, int Wc) {
  if (n < 1 || n > GE_BATCH_MAX || Hc <= 0 || Wc <= 0) return 0;
  return (size_t)n * metrics_blocks(Hc, Wc) * GE_EVAL_SUMS * sizeof(double);
}
extern "C" size_t ge_depth_metrics_workspace(int Hc, int Wc) { return ge_depth_metrics_batch_workspace(1, Hc, Wc); }

// what both KITTI entry points refuse, but for their own rule on the prediction's alignment
static int metrics_check(const float* pred, const GeBatchFrame* frames, int n, const EvalArgs& a, const double* partials, const double* sums) {
  if (!pred || !partials || !sums) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, a.Hc, a.Wc, false)) return e;                           // every window lies in its frame
  if (a.r0 < 0 || a.r0 > a.Hc || a.r1 < 0 || a.r1 > a.Hc || a.c0 < 0 || a.c0 > a.Wc || a.c1 < 0 || a.c1 > a.Wc) return GE_ERR_BAD_ARG;
  if (((uintptr_t)partials & 7) || ((uintptr_t)sums & 7)) return GE_ERR_UNSUPPORTED;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].image & 1) return GE_ERR_UNSUPPORTED;
  return GE_OK;
}
// the two launches over n checked images; pv: the prediction takes float4 loads
static int metrics_launch(const float* pred, const GeBatchFrame* frames, int n, bool pv, const EvalArgs& a, double* partials, double* sums,
                          void* stream) {
  hipStream_t s = ge_stream(stream);
  const unsigned blocks = metrics_blocks(a.Hc, a.Wc);
  const dim3 grid(blocks, (unsigned)n);
  if (pv)
    metrics_partial_k<true><<<grid, GE_EVAL_THREADS, 0, s>>>(pred, batch_table(frames, n), a, partials);
  else
    metrics_partial_k<false><<<grid, GE_EVAL_THREADS, 0, s>>>(pred, batch_table(frames, n), a, partials);
  GE_LAUNCH_CHECK();
  metrics_fold_k<<<(unsigned)n, GE_WAVE, 0, s>>>(partials, (int)blocks, sums);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" int ge_depth_metrics(const float* pred, const uint16_t* gt_raw, int H, int W, int top, int left, int Hc, int Wc,
                                int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth,
                                double* partials, double* sums, void* stream) {
  const GeBatchFrame fr = {gt_raw, nullptr, H, W, top, left};
  const EvalArgs a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  if (int e = metrics_check(pred, &fr, 1, a, partials, sums)) return e;
  if ((uintptr_t)pred & 3) return GE_ERR_UNSUPPORTED;
  return metrics_launch(pred, &fr, 1, ((uintptr_t)pred & 15) == 0 && (Wc & 3) == 0, a, partials, sums, stream);
}

extern "C" int ge_depth_metrics_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                                      float depth_scale, float min_depth, float max_depth, double* partials, double* sums, void* stream) {
  const EvalArgs a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  if (int e = metrics_check(pred, frames, n, a, partials, sums)) return e;
  if ((Wc & 3) || ((uintptr_t)pred & 15)) return GE_ERR_UNSUPPORTED;
  return metrics_launch(pred, frames, n, true, a, partials, sums, stream);
}

extern "C" int ge_depth_strata_count(int n_edges, int use_ground) {
  return n_edges < 0 || n_edges > GE_STRATA_MAX_EDGES ? 0 : (n_edges + 1) * (use_ground ? 2 : 1);
}
extern "C" size_t ge_depth_metrics_strata_workspace(int n, int Hc, int Wc, int strata) {
  if (strata < 1 || strata > GE_STRATA_MAX) return 0;
  return (size_t)strata * ge_depth_metrics_batch_workspace(n, Hc, Wc);
}

// what both strata entry points refuse beyond metrics_check, every bad argument before anything unsupported; fills `sa`
static int strata_check(const float* pred, const GeBatchFrame* frames, int n, const EvalArgs& a, const float* edges, int n_edges, float tol,
                        const double* partials, const double* sums, StratumArgs* sa) {
  const int e = metrics_check(pred, frames, n, a, partials, sums);
  if (e == GE_ERR_BAD_ARG) return e;
  if (n_edges < 0 || n_edges > GE_STRATA_MAX_EDGES || (n_edges > 0 && !edges)) return GE_ERR_BAD_ARG;
  for (int j = 0; j < n_edges; ++j)
    if (!std::isfinite(edges[j]) || (j > 0 && !(edges[j] > edges[j - 1]))) return GE_ERR_BAD_ARG;
  if (!(tol >= 0.f && tol <= 1.f)) return GE_ERR_BAD_ARG;                    // NaN fails both comparisons
  for (int f = 1; f < n; ++f)
    if (!frames[f].aux != !frames[0].aux) return GE_ERR_BAD_ARG;             // ground planes: all or none
  if (e) return e;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].aux & 3) return GE_ERR_UNSUPPORTED;
  for (int j = 0; j < GE_STRATA_MAX_EDGES; ++j) sa->e[j] = j < n_edges ? edges[j] : 0.f;
  sa->n_edges = n_edges;
  sa->C = frames[0].aux ? 2 : 1;
  sa->tol = tol;
  return GE_OK;
}
// the two launches over n checked images and S = (n_edges + 1) * C strata
static int strata_launch(const float* pred, const GeBatchFrame* frames, int n, bool pv, const EvalArgs& a, const StratumArgs& sa, double* partials,
                         double* sums, void* stream) {
  hipStream_t s = ge_stream(stream);
  const unsigned blocks = metrics_blocks(a.Hc, a.Wc), S = (unsigned)((sa.n_edges + 1) * sa.C);
  const dim3 grid(blocks, (unsigned)n, S);
  if (pv)
    metrics_strata_partial_k<true><<<grid, GE_EVAL_THREADS, 0, s>>>(pred, batch_table(frames, n), a, sa, partials);
  else
    metrics_strata_partial_k<false><<<grid, GE_EVAL_THREADS, 0, s>>>(pred, batch_table(frames, n), a, sa, partials);
  GE_LAUNCH_CHECK();
  metrics_fold_k<<<(unsigned)n * S, GE_WAVE, 0, s>>>(partials, (int)blocks, sums);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" int ge_depth_metrics_strata(const float* pred, const uint16_t* gt_raw, const float* ground, int H, int W, int top, int left, int Hc,
                                       int Wc, int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth,
                                       const float* edges, int n_edges, float ground_tol, double* partials, double* sums, void* stream) {
  const GeBatchFrame fr = {gt_raw, ground, H, W, top, left};
  const EvalArgs a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  StratumArgs sa;
  if (int e = strata_check(pred, &fr, 1, a, edges, n_edges, ground_tol, partials, sums, &sa)) return e;
  if ((uintptr_t)pred & 3) return GE_ERR_UNSUPPORTED;
  return strata_launch(pred, &fr, 1, ((uintptr_t)pred & 15) == 0 && (Wc & 3) == 0, a, sa, partials, sums, stream);
}

extern "C" int ge_depth_metrics_strata_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                                             float depth_scale, float min_depth, float max_depth, const float* edges, int n_edges,
                                             float ground_tol, double* partials, double* sums, void* stream) {
  const EvalArgs a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  StratumArgs sa;
  if (int e = strata_check(pred, frames, n, a, edges, n_edges, ground_tol, partials, sums, &sa)) return e;
  if ((Wc & 3) || ((uintptr_t)pred & 15)) return GE_ERR_UNSUPPORTED;
  return strata_launch(pred, frames, n, true, a, sa, partials, sums, stream);
}

extern "C" size_t ge_depth_metrics_resized_workspace(int H, int W) { return ge_depth_metrics_workspace(H, W); }

// the two launches over n checked images whose ground truths share (H, W) = frames[0]'s
static int metrics_resized_launch(const float* pred, int h, int w, const GeBatchFrame* frames, int n, float min_depth, float max_depth,
                                  double* partials, double* sums, void* stream) {
  hipStream_t s = ge_stream(stream);
  ResizedArgs a;
  a.h = h; a.w = w; a.H = frames[0].H; a.W = frames[0].W; a.lo = min_depth; a.hi = max_depth;
  const unsigned blocks = metrics_blocks(a.H, a.W);
  const dim3 grid(blocks, (unsigned)n);
  metrics_resized_partial_k<<<grid, GE_EVAL_THREADS, 0, s>>>(pred, batch_table(frames, n), a, partials);
  GE_LAUNCH_CHECK();
  metrics_fold_k<<<(unsigned)n, GE_WAVE, 0, s>>>(partials, (int)blocks, sums);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" int ge_depth_metrics_resized(const float* pred, int h, int w, const float* gt, int H, int W, float min_depth, float max_depth,
                                        double* partials, double* sums, void* stream) {
  if (!pred || !gt || !partials || !sums || h <= 0 || w <= 0 || H <= 0 || W <= 0) return GE_ERR_BAD_ARG;
  if (((uintptr_t)pred & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)sums & 7)) return GE_ERR_UNSUPPORTED;
  const GeBatchFrame fr = {gt, nullptr, H, W, 0, 0};
  return metrics_resized_launch(pred, h, w, &fr, 1, min_depth, max_depth, partials, sums, stream);
}

extern "C" size_t ge_depth_metrics_resized_batch_workspace(int n, int H, int W) { return ge_depth_metrics_batch_workspace(n, H, W); }

extern "C" int ge_depth_metrics_resized_batch(const float* pred, int h, int w, const GeBatchFrame* frames, int n, float min_depth,
                                              float max_depth, double* partials, double* sums, void* stream) {
  if (!pred || !partials || !sums || h <= 0 || w <= 0) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, 1, 1, false)) return e;           // the frame list itself; the whole ground truth counts: no window
  for (int f = 0; f < n; ++f)
    if (frames[f].top != 0 || frames[f].left != 0) return GE_ERR_BAD_ARG;
  for (int f = 1; f < n; ++f)
    if (frames[f].H != frames[0].H || frames[f].W != frames[0].W) return GE_ERR_UNSUPPORTED;      // one block partition for all images
  if (((uintptr_t)pred & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)sums & 7)) return GE_ERR_UNSUPPORTED;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].image & 3) return GE_ERR_UNSUPPORTED;
  return metrics_resized_launch(pred, h, w, frames, n, min_depth, max_depth, partials, sums, stream);
}
