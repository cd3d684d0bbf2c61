// Depth colorization (depth/utils/color_depth.py colorize of the reference, followed by matplotlib's Colormap.__call__(x, bytes=True)
// and the reference's [..., :3][..., ::-1]; gedepth_amd/depth/utils/color_depth.py here): depth -> normalised value -> colormap index
// -> uint8 BGR, bit for bit.
//
// The arithmetic is numpy's float32 arithmetic: x = (v - vmin) / den with a true IEEE division (no reciprocal, no contraction), or x = v * 0
// when vmin == vmax; xa = x * N; xa == N -> N - 1; then NaN -> bad (N + 2), xa < 0 -> under (N), xa >= N -> over (N + 1), else trunc(xa).
// When a bound is taken from the data (vmin / vmax None: value.min() / value.max(), NaN-propagating like numpy), ge_depth_colorize first
// runs a partial min/max pass into `minmax_ws`; every block of the colour pass folds those partials itself, so nothing synchronises with
// the host.  Colour pass: four pixels per lane (one 16-byte load, three 4-byte stores = 12 output bytes), the (N + 3)-entry table staged
// in LDS as one packed word per entry.  Pure streaming work (~1.7 MB read, 1.3 MB written at 352 x 1216): launch-latency-sized.
#pragma clang fp contract(off)
#include "common.h"

#define GE_CMAP_MAX_N 4096       // LDS table of (N + 3) words: 16.4 KB at most
#define GE_MINMAX_PARTS 256      // partial (min, max) pairs of the reduction pass = the minmax_ws size / 2

__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }   // NaN wins, like numpy.min
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// 256-thread (min, max) fold through `red` (512 floats); every thread returns the block's result
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red) {
  const int t = threadIdx.x;
  red[t] = mn; red[256 + t] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) { red[t] = nan_min(red[t], red[t + s]); red[256 + t] = nan_max(red[256 + t], red[256 + t + s]); }
    __syncthreads();
  }
  mn = red[0]; mx = red[256];
}

// pass 1 (only when a bound comes from the data): block b writes its (min, max) of a grid-stride share of src to ws[2b], ws[2b + 1]
__global__ void __launch_bounds__(256) colorize_minmax_k(const float* __restrict__ src, long n, float* __restrict__ ws) {
  __shared__ float red[512];
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = src[i];
    mn = nan_min(mn, v); mx = nan_max(mx, v);
  }
  block_minmax(mn, mx, red);
  if (threadIdx.x == 0) { ws[2 * blockIdx.x] = mn; ws[2 * blockIdx.x + 1] = mx; }
}

struct CmapArgs { float vmin, vmax, den; int flags, N, parts; };

__device__ __forceinline__ int cmap_index(float v, float lo, float den, bool eq, int N, float fN) {
  const float x = eq ? v * 0.f : (v - lo) / den;
  float xa = x * fN;
  if (xa == fN) xa = (float)(N - 1);
  if (xa != xa) return N + 2;
  if (xa < 0.f) return N;
  if (xa >= fN) return N + 1;
  return (int)xa;
}

// pass 2.  VEC: src 16-byte and dst 4-byte aligned (float4 load, three dword stores per group of 4); otherwise scalar loads, byte stores.
template <bool VEC>
__global__ void __launch_bounds__(256) colorize_k(const float* __restrict__ src, long n, CmapArgs a, const float* __restrict__ ws,
                                                  const uint8_t* __restrict__ lut_bgr, uint8_t* __restrict__ dst) {
  extern __shared__ uint32_t lut[];                 // (N + 3) entries, B | G << 8 | R << 16
  __shared__ float red[512];
  const int N = a.N;
  for (int e = threadIdx.x; e < N + 3; e += 256)
    lut[e] = (uint32_t)lut_bgr[3 * e] | ((uint32_t)lut_bgr[3 * e + 1] << 8) | ((uint32_t)lut_bgr[3 * e + 2] << 16);
  float lo = a.vmin, den = a.den;
  bool eq = (a.flags & GE_COLORIZE_EQUAL) != 0;
  if (a.flags & (GE_COLORIZE_VMIN_DATA | GE_COLORIZE_VMAX_DATA)) {
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    for (int p = threadIdx.x; p < a.parts; p += 256) { mn = nan_min(mn, ws[2 * p]); mx = nan_max(mx, ws[2 * p + 1]); }
    block_minmax(mn, mx, red);
    lo = (a.flags & GE_COLORIZE_VMIN_DATA) ? mn : a.vmin;
    const float hi = (a.flags & GE_COLORIZE_VMAX_DATA) ? mx : a.vmax;
    eq = lo == hi;                                  // numpy: float32 scalars compare (and subtract) in float32
    den = hi - lo;
  }
  __syncthreads();
  const float fN = (float)N;
  const long groups = n >> 2;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    float v[4];
    if (VEC) {
      const float4 t = *(const float4*)(src + 4 * g);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = src[4 * g + k];
    }
    uint32_t p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = lut[cmap_index(v[k], lo, den, eq, N, fN)];
    uint8_t* d = dst + 12 * g;
    if (VEC) {
      uint32_t* w = (uint32_t*)d;
      w[0] = p[0] | (p[1] << 24);
      w[1] = (p[1] >> 8) | (p[2] << 16);
      w[2] = (p[2] >> 16) | (p[3] << 8);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) { d[3 * k] = (uint8_t)p[k]; d[3 * k + 1] = (uint8_t)(p[k] >> 8); d[3 * k + 2] = (uint8_t)(p[k] >> 16); }
    }
  }
  const long e = 4 * groups + threadIdx.x;          // the n % 4 tail: block 0
  if (blockIdx.x == 0 && e < n) {
    const uint32_t q = lut[cmap_index(src[e], lo, den, eq, N, fN)];
    dst[3 * e] = (uint8_t)q; dst[3 * e + 1] = (uint8_t)(q >> 8); dst[3 * e + 2] = (uint8_t)(q >> 16);
  }
}

extern "C" int ge_depth_colorize(const float* src, long n, float vmin, float vmax, float den, int flags, float* minmax_ws,
                                 const uint8_t* lut_bgr, int N, uint8_t* dst_bgr, void* stream) {
  const int data_bounds = GE_COLORIZE_VMIN_DATA | GE_COLORIZE_VMAX_DATA;
  if (!src || !lut_bgr || !dst_bgr || n <= 0 || N <= 0 || (flags & ~(data_bounds | GE_COLORIZE_EQUAL)) ||
      ((flags & data_bounds) && !minmax_ws))
    return GE_ERR_BAD_ARG;
  if (N > GE_CMAP_MAX_N || ((uintptr_t)src & 3)) return GE_ERR_UNSUPPORTED;
  hipStream_t s = ge_stream(stream);
  CmapArgs a;
  a.vmin = vmin; a.vmax = vmax; a.den = den; a.flags = flags; a.N = N; a.parts = 0;
  if (flags & data_bounds) {
    a.parts = (int)ge_blocks(n, 256 * 16, GE_MINMAX_PARTS);
    colorize_minmax_k<<<a.parts, 256, 0, s>>>(src, n, minmax_ws);
    GE_LAUNCH_CHECK();
  }
  const unsigned blocks = ge_blocks(n >> 2, 256, 4096);
  const size_t lds = (size_t)(N + 3) * sizeof(uint32_t);
  if (((uintptr_t)src & 15) == 0 && ((uintptr_t)dst_bgr & 3) == 0)
    colorize_k<true><<<blocks, 256, lds, s>>>(src, n, a, minmax_ws, lut_bgr, dst_bgr);
  else
    colorize_k<false><<<blocks, 256, lds, s>>>(src, n, a, minmax_ws, lut_bgr, dst_bgr);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
