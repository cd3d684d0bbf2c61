// Shared device helpers for the gfx950 kernels of libgedepth_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gedepth_hip.h"

#define GE_WAVE 64

#define GE_LAUNCH_CHECK()                         \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

typedef uint16_t bf16_t;  // raw bfloat16 bits

__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
// Short vectors: MFMA operand / accumulator fragments, packed bf16 pairs (v_dot2c_f32_bf16, v_cvt_pk_bf16_f32), raw 16-byte moves
typedef __bf16 ge_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ge_bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ge_bf16x2 __attribute__((ext_vector_type(2)));
typedef float ge_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int ge_u32x4 __attribute__((ext_vector_type(4)));
typedef short ge_s16x2 __attribute__((ext_vector_type(2)));
#define GE_LDS(T, p) ((__attribute__((address_space(3))) T*)(p))   // generic -> LDS pointer, for the builtins that take address space 3

// fp32 -> bf16, round-to-nearest-even like torch, NaN stays NaN.  f2bf_hw / ge_pack_bf16x2 are ALWAYS gfx950's conversion unit
// (v_cvt_pk_bf16_f32): the MFMA kernels round their operand tiles with these whatever the build says.
__device__ __forceinline__ bf16_t f2bf_hw(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
__device__ __forceinline__ uint32_t ge_pack_bf16x2(float lo, float hi) {   // lo in bits 0-15, hi in bits 16-31
  ge_bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
// f2bf is the storage rounding of the streaming kernels (Io, Vec): the conversion unit too, unless the build defines GE_SW_BF16 (A/B switch)
__device__ __forceinline__ bf16_t f2bf(float f) {
#ifndef GE_SW_BF16
  // The integer sequence below costs ~6 VALU per value — 48 per 16-byte store of the streaming kernels: step 47.47 -> 47.12 ms same-session,
  // conv1x1_bn_act_k 505 -> 391 us (round 5); -DGE_SW_BF16 restores it (A/B)
  return f2bf_hw(f);
#endif
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}

template <typename T> struct Io;
template <> struct Io<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
  static __device__ __forceinline__ float rt(float v) { return v; }   // round-trip through storage type
};
template <> struct Io<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
  static __device__ __forceinline__ float rt(float v) { return bf2f(f2bf(v)); }
};

// N consecutive elements of the storage type <-> N fp32 registers, one memory instruction per 16 bytes (N = 4 or 8)
// (st rounds with f2bf, not ge_pack_bf16x2: these stores are what GE_SW_BF16 switches)
template <typename T, int N> struct Vec;
template <> struct Vec<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float v[4]) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  static __device__ __forceinline__ void st(float* p, const float v[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Vec<float, 8> {
  static __device__ __forceinline__ void ld(const float* p, float v[8]) { Vec<float, 4>::ld(p, v); Vec<float, 4>::ld(p + 4, v + 4); }
  static __device__ __forceinline__ void st(float* p, const float v[8]) { Vec<float, 4>::st(p, v); Vec<float, 4>::st(p + 4, v + 4); }
};
template <> struct Vec<bf16_t, 4> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float v[4]) {
    const uint2 t = *(const uint2*)p;
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float v[4]) {
    uint2 t;
    t.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    t.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *(uint2*)p = t;
  }
};
template <> struct Vec<bf16_t, 8> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float v[8]) {
    const uint4 t = *(const uint4*)p; const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float v[8]) {
    uint4 t;
    t.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16); t.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    t.z = (uint32_t)f2bf(v[4]) | ((uint32_t)f2bf(v[5]) << 16); t.w = (uint32_t)f2bf(v[6]) | ((uint32_t)f2bf(v[7]) << 16);
    *(uint4*)p = t;
  }
};
// the 16-byte member: 8 bf16 or 4 f32 per lane and instruction
template <typename T> struct V8 : Vec<T, 16 / sizeof(T)> { static constexpr int N = 16 / sizeof(T); };

// Xor-shuffle (butterfly) reduction over aligned groups of GS lanes of the wave: every lane ends up with the group's result
template <int GS, typename V, typename Op>
__device__ __forceinline__ V ge_group_reduce(V v, Op op) {
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <int GS, typename V> __device__ __forceinline__ V ge_group_sum(V v) { return ge_group_reduce<GS>(v, [](V a, V b) { return a + b; }); }
template <typename V> __device__ __forceinline__ V ge_wave_sum(V v) { return ge_group_sum<GE_WAVE>(v); }
template <typename V> __device__ __forceinline__ V ge_wave_min(V v) { return ge_group_reduce<GE_WAVE>(v, [](V a, V b) { return min(a, b); }); }
template <typename V> __device__ __forceinline__ V ge_wave_max(V v) { return ge_group_reduce<GE_WAVE>(v, [](V a, V b) { return max(a, b); }); }

// n / d, correctly rounded, for a bf16-valued n and an integer-valued d <= 8191, given r = RN(1 / d): one Newton step on q0 = n * r
// (tools/ubench/divcheck.c checks every such pair against IEEE division).  The deformable-attention kernels form sampling locations with
// it, so that every kernel of a step lands each tap in the same cell as the forward, to the bit.
__device__ __forceinline__ float ge_div_rn(float n, float d, float r) {
  const float q0 = n * r;
  return __builtin_fmaf(__builtin_fmaf(-q0, d, n), r, q0);
}

// F.interpolate(mode='bilinear') source-index rule (scale from sizes, not from scale_factor).
struct Lerp { int i0, i1; float w0, w1; };
__device__ __forceinline__ float ge_scale(int in, int out, bool align) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}
__device__ __forceinline__ Lerp ge_lerp(int dst, int in, float scale, bool align) {
  float src = align ? scale * (float)dst : fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  Lerp r;
  r.i0 = (int)src;
  if (r.i0 > in - 1) r.i0 = in - 1;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.w1 = src - (float)r.i0;
  r.w0 = 1.f - r.w1;
  return r;
}

// cv2.INTER_NEAREST as the host evaluates it (imageops.imresize): src = min(floor(dst * in / out), in - 1) in float64; ratio = in / out
__device__ __forceinline__ int ge_nearest_src(int dst, double ratio, int n_in) {
  const int s = (int)floor((double)dst * ratio);
  return s < n_in - 1 ? s : n_in - 1;
}

// cv2.INTER_AREA when shrinking (imageops._area_weights): destination cell j covers the source interval [j s, (j + 1) s), s = in / out; source
// pixel i weighs by its overlap, weights normalised per cell, float64.  [i0, i1) = the source pixels the cell touches, inv = 1 / total overlap.
__device__ __forceinline__ void ge_area_span(int j, int n_in, int n_out, int& i0, int& i1, double& lo, double& hi, double& inv) {
#pragma clang fp contract(off)
  const double s = (double)n_in / (double)n_out;
  lo = (double)j * s; hi = (double)(j + 1) * s;
  i0 = (int)floor(lo);
  i1 = (int)ceil(hi);
  if (i1 > n_in) i1 = n_in;
  double tot = 0.0;
  for (int i = i0; i < i1; ++i) tot += fmin(hi, (double)(i + 1)) - fmax(lo, (double)i);
  inv = 1.0 / tot;
}
// One destination pixel (y, x) of the area filter over an (H, W, 3) uint8 HWC image -> the three uint8-rounded averages (rint, clamp) as f32.
// Host order: out[oh, w] = sum_h Wy[oh, h] src[h, w] (float64), then out[oh, ow] = sum_w Wx[ow, w] out[oh, w].
__device__ __forceinline__ void ge_area_u8_pixel(const uint8_t* __restrict__ src, int H, int W, int Ho, int Wo, int y, int x, float out[3]) {
#pragma clang fp contract(off)
  int y0, y1, x0, x1;
  double ylo, yhi, yinv, xlo, xhi, xinv;
  ge_area_span(y, H, Ho, y0, y1, ylo, yhi, yinv);
  ge_area_span(x, W, Wo, x0, x1, xlo, xhi, xinv);
  double acc[3] = {0.0, 0.0, 0.0};
  for (int xx = x0; xx < x1; ++xx) {
    const double wx = (fmin(xhi, (double)(xx + 1)) - fmax(xlo, (double)xx)) * xinv;
    double col[3] = {0.0, 0.0, 0.0};
    for (int yy = y0; yy < y1; ++yy) {
      const double wy = (fmin(yhi, (double)(yy + 1)) - fmax(ylo, (double)yy)) * yinv;
      const uint8_t* p = src + ((long)yy * W + xx) * 3;
      col[0] += wy * (double)p[0]; col[1] += wy * (double)p[1]; col[2] += wy * (double)p[2];
    }
    acc[0] += wx * col[0]; acc[1] += wx * col[1]; acc[2] += wx * col[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (float)fmin(fmax(rint(acc[c]), 0.0), 255.0);
}

// Bilinear backward as a gather: [lo, hi] = the output indices whose taps can touch input index X, i.e. src(o) in (X - 1, X + 1), clipped to
// [0, out - 1].  floor / ceil of the interval's ends already leave one spare candidate per side against the rounding of the division, and the
// kernels recompute each candidate's weights exactly, so a spare one contributes 0.  MARGIN widens the range by that many further candidates
// per side: the generic NCHW / NHWC kernels have always run with 1, the decoder's up-sample-and-concat with 0 (5 instead of 7 candidates at
// factor 2).  Nothing in the code shows a case that needs the second spare; the difference is preserved, not explained.
template <int MARGIN>
__device__ __forceinline__ void ge_cand_range(int X, int out, float scale, bool align, int& lo, int& hi) {
  if (scale <= 0.f) { lo = 0; hi = out - 1; return; }
  float a, b;
  if (align) { a = ((float)X - 1.f) / scale; b = ((float)X + 1.f) / scale; }
  else { a = ((float)X - 0.5f) / scale - 0.5f; b = ((float)X + 1.5f) / scale - 0.5f; }
  lo = (int)floorf(a) - MARGIN;
  hi = (int)ceilf(b) + MARGIN;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
}

static inline hipStream_t ge_stream(void* s) { return (hipStream_t)s; }

// Compute-unit count of the CURRENT device, cached per device id (a process may drive several devices; a single cached value would size the
// persistent grids of every device after the first caller's).  0 on error.
static inline int ge_cu_count() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  if (dev < 64 && __atomic_load_n(&cache[dev], __ATOMIC_RELAXED)) return cache[dev];
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
  if (dev < 64) __atomic_store_n(&cache[dev], p.multiProcessorCount, __ATOMIC_RELAXED);
  return p.multiProcessorCount;
}

// Dropout masks are a counter-based hash of (seed, element index) with the seed a launch ARGUMENT — frozen when the launch is captured in a
// hipGraph.  ge_rng_salt(ptr) (neck.hip) registers a device counter that every dropout kernel adds to its seed at EXECUTION time; a
// captured step increments it inside the graph, so each replay draws fresh masks (forward and backward of one step read the same value).
const unsigned long long* ge_rng_salt_get();
__device__ __forceinline__ uint64_t ge_salted(uint64_t seed, const unsigned long long* salt) {
  return salt ? seed + (uint64_t)*salt * 0x9E3779B97F4A7C15ull : seed;
}
// Dropout keep decisions: ONE 64-bit hash (splitmix64 finaliser) per group of four consecutive element indices, 16 bits per element:
// element idx is kept when bits [16 (idx & 3), +16) of hash(seed, idx >> 2) are >= thr = round(p * 65536) (keep probability 1 - thr / 65536: p = 0.1 ->
// 0.899994).  The per-element 32-bit hash of rounds 2 - 4 (seven multiplies and a dozen shifts / xors per value) cost the cross-attention's concat /
// slice passes 0.22 ms per step; the streaming kernels take whole groups (ge_drop_scale4), the transposing ones single elements.
__device__ __forceinline__ uint64_t ge_drop_hash4(uint64_t seed, uint64_t group) {
  uint64_t z = group * 0x9E3779B97F4A7C15ull + seed;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t ge_drop_threshold(float p) { return (uint32_t)(p * 65536.f + 0.5f); }
__device__ __forceinline__ float ge_drop_scale(uint64_t seed, uint64_t idx, uint32_t thr, float inv_keep) {
  const uint32_t u = (uint32_t)(ge_drop_hash4(seed, idx >> 2) >> (16 * (unsigned)(idx & 3))) & 0xffffu;
  return u >= thr ? inv_keep : 0.f;
}
__device__ __forceinline__ void ge_drop_scale4(uint64_t seed, uint64_t group, uint32_t thr, float inv_keep, float s[4]) {
  const uint64_t h = ge_drop_hash4(seed, group);
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = (((uint32_t)(h >> (16 * e))) & 0xffffu) >= thr ? inv_keep : 0.f;
}
static inline unsigned ge_blocks(long n, int per_block, long cap = 1 << 20) {
  long b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}
