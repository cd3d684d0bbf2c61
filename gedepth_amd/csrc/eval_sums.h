// The metric sums' device code shared by eval.hip (one image per launch) and infer_batch.hip (ge_depth_metrics_batch: up to eight images per
// launch): the pixel's ten terms, the lane's walk over the crop and the workgroup's fold.  Both callers run these very functions over the
// same block partition, which is why a batched row carries the bits of the single-image call.
#pragma once
#include "common.h"

#define GE_EVAL_THREADS 256
#define GE_EVAL_GROUPS 2           // groups of four pixels per lane before the grid-stride loop goes round again
#define GE_EVAL_MAX_BLOCKS 1024
#define GE_EVAL_SUMS 10

struct EvalArgs { int W, top, left, Hc, Wc, r0, r1, c0, c1; float scale, lo, hi; };

// One pixel: `gt` in metres (f32), `inside` = it lies in the protocol's rectangle; it counts when also lo < gt < hi.
__device__ __forceinline__ void metric_pixel(float p, float gt, bool inside, float lo, float hi, double acc[GE_EVAL_SUMS]) {
#pragma clang fp contract(off)
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

// One lane's sums over the crop of one image, as workgroup blockIdx.x of gridDim.x.
// PV: pred is 16-byte aligned and Wc % 4 == 0 (one float4 per group).  GV (only with PV): every group's four ground-truth values are
// 8-byte aligned (W % 4 == 0, left % 4 == 0, base 8-byte aligned).  Otherwise element loads, each one bounds-checked against Wc.
template <bool PV, bool GV>
__device__ __forceinline__ void metrics_window_sums(const float* __restrict__ pred, const uint16_t* __restrict__ gt_raw, const EvalArgs& a,
                                                    double acc[GE_EVAL_SUMS]) {
#pragma clang fp contract(off)
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
    for (int k = 0; k < 4; ++k)                                                   // gt = (float)raw / depth_scale; c1 <= Wc covers the row's tail
      metric_pixel(p[k], (float)raw[k] / a.scale, c + k >= a.c0 && c + k < a.c1, a.lo, a.hi, acc);
  }
}

static inline unsigned metrics_blocks(int Hc, int Wc) {
  return ge_blocks((long)Hc * ((Wc + 3) >> 2), GE_EVAL_THREADS * GE_EVAL_GROUPS, GE_EVAL_MAX_BLOCKS);
}
