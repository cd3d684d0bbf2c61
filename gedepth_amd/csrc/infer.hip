// KITTI / DDAD inference (depth/apis/inference.py of the reference; gedepth_amd/depth/apis/inference.py and batch_inference.py here): the
// test pipeline's per-frame front end and the flip-TTA merge of encoder_decoder.py aug_test, each as one streaming launch around the
// forward of the flip views.  The kernels take up to GE_BATCH_MAX frames per launch, the frame index on blockIdx.y
// (include/gedepth_batch.h, include/gedepth_ddad_batch.h); the single-frame entry points of gedepth_hip.h and gedepth_ddad.h are their
// launch of one frame.
//
// The KITTI front end restates, op for op, LoadImageFromFile(USEPE) -> KBCrop -> MultiScaleFlipAug(RandomFlip, Normalize) of
// configs/_base_/datasets/kitti_gedepth.py, i.e. the composition ge_aug_load -> ge_aug_color_normalize(color_on = 0) ->
// ge_aug_window(flip) of aug.hip, so that both produce the same bits.  Each thread reads four consecutive pixels of the crop window
// once and writes them to view 0 and, reversed, to the mirrored position of view 1: one read of the window, 16-byte stores to both
// views, no LDS.  Pure streaming work (~3.3 MB read, 17.1 MB written per frame): launch-latency-sized, no MFMA.
// The prior sweep's front end (include/gedepth_sweep.h) is the same thread with a loop over ground-prior variants around its stores.
#pragma clang fp contract(off)
#include "batch_table.h"
#include "../../include/gedepth_ddad.h"
#include "../../include/gedepth_ddad_batch.h"
#include "../../include/gedepth_sweep.h"
#include <cmath>

struct InferNorm { double mean[3], stdinv[3]; float pe_max, depth_scale; int to_rgb; };
static InferNorm infer_norm(float pe_max, const double* mean3, const double* std3, float depth_scale, int to_rgb) {
  InferNorm p;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.stdinv[c] = 1.0 / std3[c]; }
  p.pe_max = pe_max; p.depth_scale = depth_scale; p.to_rgb = to_rgb;
  return p;
}

extern "C" size_t ge_batch_frame_size(void) { return sizeof(GeBatchFrame); }

// What a thread of the KITTI front ends does for its four consecutive pixels, shared by infer_front_k and infer_front_sweep_k so that
// the two cannot drift.  front_pixel: pixel k of the four -> column k of o.  COLOUR: the three bytes at px -> rows 0 .. 2 (ge_aug_load:
// (float)u8; ge_aug_color_normalize: truncf, a no-op on a uint8 value, BGR -> RGB, f64 (x - mean) * (1 / std)).  GROUND: the raw ground
// depth -> row 3 (LoadImageFromFile: > pe_max or < 0 zeroed; Normalize: / depth_scale where > 0) and row 4 (the value itself).
// infer_front_k does both per pixel; the sweep does COLOUR once and GROUND once per variant.  front_store: the five 16-byte rows to
// view 0 and, reversed, to the mirrored position of view 1 (ge_aug_window(flip): x -> Wc - 1 - x); n = Hc * Wc, r = y * Wc.
template <bool COLOUR, bool GROUND>
__device__ __forceinline__ void front_pixel(const uint8_t* __restrict__ px, float raw, const InferNorm& p, int k, float (&o)[5][4]) {
  if (COLOUR) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = truncf((float)px[c]);
      const int oc = p.to_rgb ? 2 - c : c;
      o[oc][k] = (float)(((double)v - p.mean[oc]) * p.stdinv[oc]);
    }
  }
  if (GROUND) {
    float f = raw;
    if (f > p.pe_max) f = 0.f;
    if (f < 0.f) f = 0.f;
    if (f > 0.f) f = f / p.depth_scale;
    o[3][k] = f;
    o[4][k] = raw;
  }
}
__device__ __forceinline__ void front_store(float* __restrict__ dst, long n, long r, int g, int Wc, int views, const float (&o)[5][4]) {
#pragma unroll
  for (int c = 0; c < 5; ++c) *(float4*)(dst + c * n + r + 4 * g) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  if (views == 2) {
    float* d1 = dst + 5 * n + r + (Wc - 4 - 4 * g);
#pragma unroll
    for (int c = 0; c < 5; ++c) *(float4*)(d1 + c * n) = make_float4(o[c][3], o[c][2], o[c][1], o[c][0]);
  }
}

// Frame f = blockIdx.y of the table (batch_table.h) -> images views * f .. views * f + views - 1 of dst (views * n, 5, Hc, Wc) planar f32;
// view 1 = view 0 mirrored horizontally.  Wc % 4 == 0, dst 16-byte aligned (checked by the caller).  The frames share grid.x, so a frame's
// bits do not depend on how many frames the launch has: ge_infer_front is the launch of one.
__global__ void __launch_bounds__(256) infer_front_k(BatchTable t, float* __restrict__ dst, int Hc, int Wc, int views, InferNorm p) {
  const GeBatchFrame fr = t.f[blockIdx.y];
  const uint8_t* __restrict__ bgr = (const uint8_t*)fr.image;
  const float* __restrict__ pe = (const float*)fr.aux;
  const int G = Wc >> 2;                                   // float4 groups per output row
  const long n = (long)Hc * Wc, groups = (long)Hc * G;
  dst += (long)blockIdx.y * views * 5 * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    const int y = (int)(i / G), g = (int)(i - (long)y * G);
    const long s = (long)(y + fr.top) * fr.W + (fr.left + 4 * g);
    const uint8_t* px = bgr + s * 3;
    float o[5][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) front_pixel<true, true>(px + 3 * k, pe[s + k], p, k, o);
    front_store(dst, n, (long)y * Wc, g, Wc, views, o);
  }
}
// the launch of n checked frames
static int infer_front_launch(const GeBatchFrame* frames, int n, float* dst, int Hc, int Wc, int views, const InferNorm& p, void* stream) {
  const dim3 grid(ge_blocks((long)Hc * (Wc / 4), 256, 65536), (unsigned)n);
  infer_front_k<<<grid, 256, 0, ge_stream(stream)>>>(batch_table(frames, n), dst, Hc, Wc, views, p);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
extern "C" int ge_infer_front(const uint8_t* bgr_hwc, const float* pe, float* dst, int H, int W, int top, int left, int Hc, int Wc,
                              int views, float pe_max, const double* mean3, const double* std3, float depth_scale, int to_rgb,
                              void* stream) {
  if (!bgr_hwc || !pe || !dst || !mean3 || !std3 || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0 || top < 0 || left < 0 || top + Hc > H ||
      left + Wc > W || (views != 1 && views != 2))
    return GE_ERR_BAD_ARG;
  if ((Wc & 3) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;          // (the ground depth's alignment: ge_infer_front_batch only)
  const GeBatchFrame fr = {bgr_hwc, pe, H, W, top, left};
  return infer_front_launch(&fr, 1, dst, Hc, Wc, views, infer_norm(pe_max, mean3, std3, depth_scale, to_rgb), stream);
}
extern "C" int ge_infer_front_batch(const GeBatchFrame* frames, int n, float* dst, int Hc, int Wc, int views, float pe_max,
                                    const double* mean3, const double* std3, float depth_scale, int to_rgb, void* stream) {
  if (!dst || !mean3 || !std3 || (views != 1 && views != 2)) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, Hc, Wc, true)) return e;
  if ((Wc & 3) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].aux & 3) return GE_ERR_UNSUPPORTED;
  return infer_front_launch(frames, n, dst, Hc, Wc, views, infer_norm(pe_max, mean3, std3, depth_scale, to_rgb), stream);
}

// The prior sweep (include/gedepth_sweep.h): one frame -> nv slots that differ only in channels 3 and 4.  prior_variant is the header's
// rule, branch for branch; the baseline (c == 0, s == 1) hands the plane through, since 1 / (1 / pe) is not pe in f32.
__device__ __forceinline__ float prior_variant(float pe, const GePriorVariant& v) {
  if (v.drop) return 0.f;
  if (v.c == 0.f && v.s == 1.f) return pe;
  if (!(pe > 0.f)) return pe;
  const float q = 1.f / pe + v.c;
  return q > 0.f ? v.s / q : 0.f;
}
struct SweepTable { GePriorVariant v[GE_SWEEP_MAX]; };
static_assert(sizeof(GePriorVariant) == 12 && sizeof(SweepTable) == 96, "the by-value variant table is 8 x {two floats, one int}");

// Variant v of the table -> images views * v .. views * v + views - 1 of dst (views * nv, 5, Hc, Wc) planar f32, each with the bits
// infer_front_k writes for the plane prior_variant(pe, v).  The variants are the INNER loop of a thread: it reads its twelve colour bytes
// and four ground depths once, normalises the colour once (the float64 part of the work) and keeps the sixteen values in registers; per
// variant it forms eight values and issues the ten 16-byte stores.  With the variants on blockIdx.y instead the frame would be read and
// normalised nv times; here the launch reads ~3.3 MB once and writes 17.1 MB per variant.  The table is read at a uniform index (scalar
// loads from the kernel-argument block).  No LDS, no atomics; Wc % 4 == 0, dst 16-byte aligned (checked by the caller).
__global__ void __launch_bounds__(256) infer_front_sweep_k(const uint8_t* __restrict__ bgr, const float* __restrict__ pe, int W, int top,
                                                           int left, SweepTable t, int nv, float* __restrict__ dst, int Hc, int Wc, int views,
                                                           InferNorm p) {
  const int G = Wc >> 2;
  const long n = (long)Hc * Wc, groups = (long)Hc * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    const int y = (int)(i / G), g = (int)(i - (long)y * G);
    const long s = (long)(y + top) * W + (left + 4 * g);
    const uint8_t* px = bgr + s * 3;
    float o[5][4], raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      front_pixel<true, false>(px + 3 * k, 0.f, p, k, o);
      raw[k] = pe[s + k];
    }
    for (int v = 0; v < nv; ++v) {
      const GePriorVariant var = t.v[v];
#pragma unroll
      for (int k = 0; k < 4; ++k) front_pixel<false, true>(px, prior_variant(raw[k], var), p, k, o);
      front_store(dst + (long)v * views * 5 * n, n, (long)y * Wc, g, Wc, views, o);
    }
  }
}
extern "C" size_t ge_prior_variant_size(void) { return sizeof(GePriorVariant); }
extern "C" int ge_infer_front_sweep(const uint8_t* bgr_hwc, const float* pe, int H, int W, int top, int left, const GePriorVariant* variants,
                                    int n, float* dst, int Hc, int Wc, int views, float pe_max, const double* mean3, const double* std3,
                                    float depth_scale, int to_rgb, void* stream) {
  if (!bgr_hwc || !pe || !variants || !dst || !mean3 || !std3 || n < 1 || n > GE_SWEEP_MAX || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0 ||
      top < 0 || left < 0 || Hc > H - top || Wc > W - left || (views != 1 && views != 2))
    return GE_ERR_BAD_ARG;
  SweepTable t;
  for (int v = 0; v < GE_SWEEP_MAX; ++v) t.v[v] = variants[v < n ? v : 0];      // entries >= n are never read
  for (int v = 0; v < n; ++v)
    if (!std::isfinite(t.v[v].c) || !std::isfinite(t.v[v].s) || !(t.v[v].s > 0.f)) return GE_ERR_BAD_ARG;
  if ((Wc & 3) || ((uintptr_t)dst & 15) || ((uintptr_t)pe & 3)) return GE_ERR_UNSUPPORTED;
  const unsigned grid = ge_blocks((long)Hc * (Wc / 4), 256, 65536);
  infer_front_sweep_k<<<grid, 256, 0, ge_stream(stream)>>>(bgr_hwc, pe, W, top, left, t, n, dst, Hc, Wc, views,
                                                          infer_norm(pe_max, mean3, std3, depth_scale, to_rgb));
  GE_LAUNCH_CHECK();
  return GE_OK;
}

// ge_infer_front_ddad restates LoadDDADImageFromFile(USEPE, USE_DYNAMIC_PE) -> DDADResize(shape, depth = False) -> Normalize of
// configs/_base_/datasets/ddad_gedepth.py, i.e. the composition the training pipeline runs (DDADGPUPipeline._front): ge_aug_area_u8, the
// nearest ge_aug_resize of (clamped pe, raw pe), ge_aug_color_normalize(color_on = 0) — through the same device functions (common.h), so
// that both produce the same bits.  Each thread forms four consecutive output pixels: 3 x 3 (DDAD: 1216 x 1936 -> 384 x 640, factor
// 3.17 x 3.03, up to 4 x 4 + edges) source pixels each in float64, two gathers of the ground depth, five 16-byte stores.
// The output array is indexed by `oc` (BGR -> RGB), which the compiler resolves into selects: 77 VGPRs, no scratch.  The row span of the
// area filter is formed again for each of the four pixels, inside the shared ge_area_u8_pixel: one launch per frame of 7 680 threads
// (384 x 640), sized by launch latency, so the shared function stays whole rather than being split for this caller.
// Frame f = blockIdx.y of the table (batch_table.h; `image` the frame, `aux` its camera's ground depth, H and W its own) -> image f of dst
// (n, 5, Hd, Wd) planar f32; Wd % 4 == 0, dst 16-byte aligned (checked by the caller).  The frames share grid.x, so a frame's bits do not
// depend on how many frames the launch has: ge_infer_front_ddad is the launch of one (include/gedepth_ddad_batch.h).
__global__ void __launch_bounds__(256) infer_front_ddad_k(BatchTable t, float* __restrict__ dst, int Hd, int Wd, InferNorm p) {
  const GeBatchFrame fr = t.f[blockIdx.y];
  const uint8_t* __restrict__ bgr = (const uint8_t*)fr.image;
  const float* __restrict__ pe = (const float*)fr.aux;
  const int H = fr.H, W = fr.W;
  const int G = Wd >> 2;
  const long n = (long)Hd * Wd, groups = (long)Hd * G;
  const double dy = (double)H / (double)Hd, dx = (double)W / (double)Wd;
  dst += (long)blockIdx.y * 5 * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    const int y = (int)(i / G), g = (int)(i - (long)y * G);
    const int ys = ge_nearest_src(y, dy, H);                // aug_resize_k mode 0
    float o[5][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = 4 * g + k;
      float v[3];
      ge_area_u8_pixel(bgr, H, W, Hd, Wd, y, x, v);         // aug_area_u8_k
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = truncf(v[c]);                       // aug_color_k: a no-op on a uint8 value; BGR -> RGB, f64 (x - mean) * (1 / std)
        const int oc = p.to_rgb ? 2 - c : c;
        o[oc][k] = (float)(((double)u - p.mean[oc]) * p.stdinv[oc]);
      }
      const float raw = pe[(long)ys * W + ge_nearest_src(x, dx, W)];
      float f = raw;                                        // LoadDDADImageFromFile: > pe_max or < 0 zeroed; Normalize: / depth_scale where > 0
      if (f > p.pe_max) f = 0.f;
      if (f < 0.f) f = 0.f;
      if (f > 0.f) f = f / p.depth_scale;
      o[3][k] = f;
      o[4][k] = raw;
    }
    const long r = (long)y * Wd + 4 * g;
#pragma unroll
    for (int c = 0; c < 5; ++c) *(float4*)(dst + c * n + r) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  }
}
// the launch of n checked frames
static int infer_front_ddad_launch(const GeBatchFrame* frames, int n, float* dst, int Hd, int Wd, const InferNorm& p, void* stream) {
  const dim3 grid(ge_blocks((long)Hd * (Wd / 4), 256, 65536), (unsigned)n);
  infer_front_ddad_k<<<grid, 256, 0, ge_stream(stream)>>>(batch_table(frames, n), dst, Hd, Wd, p);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
extern "C" int ge_infer_front_ddad(const uint8_t* bgr_hwc, const float* pe, float* dst, int H, int W, int Hd, int Wd, float pe_max,
                                   const double* mean3, const double* std3, float depth_scale, int to_rgb, void* stream) {
  if (!bgr_hwc || !pe || !dst || !mean3 || !std3 || H <= 0 || W <= 0 || Hd <= 0 || Wd <= 0) return GE_ERR_BAD_ARG;
  if (Hd > H || Wd > W) return GE_ERR_UNSUPPORTED;          // the area filter is the shrinking branch, as in ge_aug_area_u8
  if ((Wd & 3) || ((uintptr_t)dst & 15) || ((uintptr_t)pe & 3)) return GE_ERR_UNSUPPORTED;
  const GeBatchFrame fr = {bgr_hwc, pe, H, W, 0, 0};
  return infer_front_ddad_launch(&fr, 1, dst, Hd, Wd, infer_norm(pe_max, mean3, std3, depth_scale, to_rgb), stream);
}
extern "C" int ge_infer_front_ddad_batch(const GeBatchFrame* frames, int n, float* dst, int Hd, int Wd, float pe_max, const double* mean3,
                                         const double* std3, float depth_scale, int to_rgb, void* stream) {
  if (!dst || !mean3 || !std3 || Hd <= 0 || Wd <= 0) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, 1, 1, true)) return e;            // the frame list itself; the whole frame is resized: no window
  for (int f = 0; f < n; ++f)
    if (frames[f].top != 0 || frames[f].left != 0) return GE_ERR_BAD_ARG;
  for (int f = 0; f < n; ++f)
    if (Hd > frames[f].H || Wd > frames[f].W) return GE_ERR_UNSUPPORTED;      // the area filter is the shrinking branch
  if ((Wd & 3) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].aux & 3) return GE_ERR_UNSUPPORTED;
  return infer_front_ddad_launch(frames, n, dst, Hd, Wd, infer_norm(pe_max, mean3, std3, depth_scale, to_rgb), stream);
}

// encoder_decoder.py aug_test over the two flip views: (out0 + flip(out1)) / 2, in that order (sum, then divide by the view count;
// the division by 2 is exact).  Frame f = blockIdx.y: src (2 n, H, W) f32, frame-major, dst (n, H, W) f32; W % 4 == 0, both 16-byte aligned.
__global__ void __launch_bounds__(256) tta_merge_k(const float* __restrict__ src, float* __restrict__ dst, int H, int W) {
  const int G = W >> 2;
  const long n = (long)H * W, groups = (long)H * G;
  src += (long)blockIdx.y * 2 * n;
  dst += (long)blockIdx.y * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
    const int y = (int)(i / G), g = (int)(i - (long)y * G);
    const long r = (long)y * W;
    const float4 a = *(const float4*)(src + r + 4 * g);
    const float4 b = *(const float4*)(src + n + r + (W - 4 - 4 * g));
    *(float4*)(dst + r + 4 * g) = make_float4((a.x + b.w) / 2.f, (a.y + b.z) / 2.f, (a.z + b.y) / 2.f, (a.w + b.x) / 2.f);
  }
}
extern "C" int ge_tta_merge_batch(const float* src, float* dst, int n, int H, int W, void* stream) {
  if (!src || !dst || n < 1 || n > GE_BATCH_MAX || H <= 0 || W <= 0) return GE_ERR_BAD_ARG;
  if ((W & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  const dim3 grid(ge_blocks((long)H * (W / 4), 256, 65536), (unsigned)n);
  tta_merge_k<<<grid, 256, 0, ge_stream(stream)>>>(src, dst, H, W);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
extern "C" int ge_tta_merge(const float* src, float* dst, int H, int W, void* stream) { return ge_tta_merge_batch(src, dst, 1, H, W, stream); }
