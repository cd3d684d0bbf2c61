// Metric sums of the KITTI evaluation protocol on the device (include/gedepth_eval.h; depth/core/evaluation.py `calculate` behind
// depth/datasets/kitti.py `pre_eval`): one image leaves the GPU as ten f64 numbers.
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
#include "common.h"
#include "../../include/gedepth_eval.h"

#define GE_EVAL_THREADS 256
#define GE_EVAL_GROUPS 2           // groups of four pixels per lane before the grid-stride loop goes round again
#define GE_EVAL_MAX_BLOCKS 1024
#define GE_EVAL_SUMS 10

struct EvalArgs { int W, top, left, Hc, Wc, r0, r1, c0, c1; float scale, lo, hi; };

__device__ __forceinline__ void metric_pixel(float p, uint16_t raw, bool inside, const EvalArgs& a, double acc[GE_EVAL_SUMS]) {
  const float gt = (float)raw / a.scale;
  if (!(inside && gt > a.lo && gt < a.hi)) return;
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

// PV: pred is 16-byte aligned and Wc % 4 == 0 (one float4 per group).  GV (only with PV): every group's four ground-truth values are
// 8-byte aligned (W % 4 == 0, left % 4 == 0, base 8-byte aligned).  Otherwise element loads, each one bounds-checked against Wc.
template <bool PV, bool GV>
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_partial_k(const float* __restrict__ pred, const uint16_t* __restrict__ gt_raw,
                                                                     EvalArgs a, double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  const int G = (a.Wc + 3) >> 2;                                      // groups per row
  const long items = (long)a.Hc * G;
  for (long it = (long)blockIdx.x * GE_EVAL_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * GE_EVAL_THREADS) {
    const int r = (int)(it / G), c = 4 * (int)(it - (long)r * G);
    if (r < a.r0 || r >= a.r1 || c + 4 <= a.c0 || c >= a.c1) continue;        // nothing of this group is in the rectangle: no loads
    const float* ps = pred + (long)r * a.Wc + c;
    const uint16_t* gs = gt_raw + (long)(a.top + r) * a.W + a.left + c;
    float p[4];
    uint16_t raw[4];
    if (PV) {
      const float4 t = *(const float4*)ps;
      p[0] = t.x; p[1] = t.y; p[2] = t.z; p[3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = c + k < a.Wc ? ps[k] : 1.f;
    }
    if (PV && GV) {
      const uint2 t = *(const uint2*)gs;
      raw[0] = (uint16_t)t.x; raw[1] = (uint16_t)(t.x >> 16); raw[2] = (uint16_t)t.y; raw[3] = (uint16_t)(t.y >> 16);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) raw[k] = c + k < a.Wc ? gs[k] : (uint16_t)0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) metric_pixel(p[k], raw[k], c + k >= a.c0 && c + k < a.c1, a, acc);    // c1 <= Wc covers the row's tail
  }
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
    partials[(long)blockIdx.x * GE_EVAL_SUMS + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(GE_WAVE) metrics_fold_k(const double* __restrict__ partials, int blocks, double* __restrict__ sums) {
  if (threadIdx.x >= GE_EVAL_SUMS) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += partials[(long)b * GE_EVAL_SUMS + threadIdx.x];
  sums[threadIdx.x] = s;
}

static inline unsigned metrics_blocks(int Hc, int Wc) {
  return ge_blocks((long)Hc * ((Wc + 3) >> 2), GE_EVAL_THREADS * GE_EVAL_GROUPS, GE_EVAL_MAX_BLOCKS);
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
