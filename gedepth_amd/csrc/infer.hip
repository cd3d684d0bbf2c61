// Single-frame inference (depth/apis/inference.py of the reference; gedepth_amd/depth/apis/inference.py here): the KITTI test
// pipeline's per-frame front end and the flip-TTA merge of encoder_decoder.py aug_test, each as one streaming launch around the
// batch-2 forward of the two flip views.
//
// ge_infer_front restates, op for op, LoadImageFromFile(USEPE) -> KBCrop -> MultiScaleFlipAug(RandomFlip, Normalize) of
// configs/_base_/datasets/kitti_gedepth.py, i.e. the composition ge_aug_load -> ge_aug_color_normalize(color_on = 0) ->
// ge_aug_window(flip) of aug.hip, so that both produce the same bits.  Each thread reads four consecutive pixels of the crop window
// once and writes them to view 0 and, reversed, to the mirrored position of view 1: one read of the window, 16-byte stores to both
// views, no LDS.  Pure streaming work (~3.3 MB read, 17.1 MB written per frame): launch-latency-sized, no MFMA.
#pragma clang fp contract(off)
#include "common.h"
#include "../../include/gedepth_ddad.h"

// dst (views, 5, Hc, Wc) planar f32; view 1 = view 0 mirrored horizontally.  Wc % 4 == 0, dst 16-byte aligned (checked by the caller).
// The group's body is ge_infer_front_group of common.h, which ge_infer_front_batch (infer_batch.hip) runs per frame too.
__global__ void __launch_bounds__(256) infer_front_k(const uint8_t* __restrict__ bgr, const float* __restrict__ pe, float* __restrict__ dst,
                                                     int W, int top, int left, int Hc, int Wc, int views, InferNorm p) {
  const int G = Wc >> 2;                                   // float4 groups per output row
  const long n = (long)Hc * Wc, groups = (long)Hc * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256)
    ge_infer_front_group(bgr, pe, dst, W, top, left, Wc, views, p, i, G, n);
}
extern "C" int ge_infer_front(const uint8_t* bgr_hwc, const float* pe, float* dst, int H, int W, int top, int left, int Hc, int Wc,
                              int views, float pe_max, const double* mean3, const double* std3, float depth_scale, int to_rgb,
                              void* stream) {
  if (!bgr_hwc || !pe || !dst || !mean3 || !std3 || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0 || top < 0 || left < 0 || top + Hc > H ||
      left + Wc > W || (views != 1 && views != 2))
    return GE_ERR_BAD_ARG;
  if ((Wc & 3) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  InferNorm p;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.stdinv[c] = 1.0 / std3[c]; }
  p.pe_max = pe_max; p.depth_scale = depth_scale; p.to_rgb = to_rgb;
  const long groups = (long)Hc * (Wc / 4);
  infer_front_k<<<ge_blocks(groups, 256, 65536), 256, 0, ge_stream(stream)>>>(bgr_hwc, pe, dst, W, top, left, Hc, Wc, views, p);
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
// dst (1, 5, Hd, Wd) planar f32; Wd % 4 == 0, dst 16-byte aligned (checked by the caller).
__global__ void __launch_bounds__(256) infer_front_ddad_k(const uint8_t* __restrict__ bgr, const float* __restrict__ pe, float* __restrict__ dst,
                                                          int H, int W, int Hd, int Wd, InferNorm p) {
  const int G = Wd >> 2;
  const long n = (long)Hd * Wd, groups = (long)Hd * G;
  const double dy = (double)H / (double)Hd, dx = (double)W / (double)Wd;
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
        const float t = truncf(v[c]);                       // aug_color_k: a no-op on a uint8 value; BGR -> RGB, f64 (x - mean) * (1 / std)
        const int oc = p.to_rgb ? 2 - c : c;
        o[oc][k] = (float)(((double)t - p.mean[oc]) * p.stdinv[oc]);
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
extern "C" int ge_infer_front_ddad(const uint8_t* bgr_hwc, const float* pe, float* dst, int H, int W, int Hd, int Wd, float pe_max,
                                   const double* mean3, const double* std3, float depth_scale, int to_rgb, void* stream) {
  if (!bgr_hwc || !pe || !dst || !mean3 || !std3 || H <= 0 || W <= 0 || Hd <= 0 || Wd <= 0) return GE_ERR_BAD_ARG;
  if (Hd > H || Wd > W) return GE_ERR_UNSUPPORTED;          // the area filter is the shrinking branch, as in ge_aug_area_u8
  if ((Wd & 3) || ((uintptr_t)dst & 15) || ((uintptr_t)pe & 3)) return GE_ERR_UNSUPPORTED;
  InferNorm p;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.stdinv[c] = 1.0 / std3[c]; }
  p.pe_max = pe_max; p.depth_scale = depth_scale; p.to_rgb = to_rgb;
  const long groups = (long)Hd * (Wd / 4);
  infer_front_ddad_k<<<ge_blocks(groups, 256, 65536), 256, 0, ge_stream(stream)>>>(bgr_hwc, pe, dst, H, W, Hd, Wd, p);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

// encoder_decoder.py aug_test over the two flip views: (out0 + flip(out1)) / 2, in that order (sum, then divide by the view count;
// the division by 2 is exact).  src (2, H, W) f32, dst (H, W) f32; W % 4 == 0, both 16-byte aligned.
__global__ void __launch_bounds__(256) tta_merge_k(const float* __restrict__ src, float* __restrict__ dst, int H, int W) {
  const int G = W >> 2;
  const long n = (long)H * W, groups = (long)H * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) ge_tta_merge_group(src, dst, W, i, G, n);
}
extern "C" int ge_tta_merge(const float* src, float* dst, int H, int W, void* stream) {
  if (!src || !dst || H <= 0 || W <= 0) return GE_ERR_BAD_ARG;
  if ((W & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  tta_merge_k<<<ge_blocks((long)H * (W / 4), 256, 65536), 256, 0, ge_stream(stream)>>>(src, dst, H, W);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
