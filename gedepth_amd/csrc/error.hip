// Where in the picture a KITTI prediction is wrong (include/gedepth_error.h): ge_error_image[_batch] paints every LiDAR return of a frame
// with the band of its abs-rel error, dilated by a (2 R + 1)^2 maximum, over the frame's own pixels; ge_error_accumulate[_batch] adds the
// abs-rel error of every return into per-pixel f64 sums and uint32 counts over a split.  The counted pixels are ge_depth_metrics' (eval.hip):
// gt = (float)raw / depth_scale, inside the rectangle, lo < gt < hi; e = fabsf(gt - p) / gt and n = e / tau are true IEEE divisions.
//
// The image kernel is tiled: a workgroup owns ERR_TH x ERR_TW output pixels.  It walks its tile plus a halo of R rows and one group of four
// columns on each side in groups of four ground-truth values, forms e and n ONCE per counted pixel (not (2 R + 1)^2 times) and stages n in
// LDS, -1.f standing for "no source" (every real n is >= 0, a NaN n became +inf, so the maximum never sees a NaN).  A group without a
// counted pixel loads no prediction.  The maximum is separable: a row pass over the staged rows into a second LDS plane, then a column
// pass per output group of four pixels, which looks up the bands and stores twelve bytes.  A tile that no source can reach (all of it more
// than R away from the rectangle) stages nothing and copies the background.  Within an LDS row consecutive lanes read and write consecutive
// 16-byte slots (row strides of 136 and 128 dwords; a wave spans two rows, so the slots are not consecutive at its row change): few bank
// conflicts are expected from this layout; none were counted, the kernel has not been profiled with hardware counters.
// The frame sits on blockIdx.y and the tile on blockIdx.x; ge_error_image is the launch of one frame with the same grid.x, so a frame has
// the same bytes alone and in a batch.  Nothing here adds floats across pixels, so there is no order to keep in the image; the
// accumulators keep theirs by ownership: a thread owns four pixels and walks the call's frames in index order, no atomics.
#pragma clang fp contract(off)
#include "batch_table.h"
#include "../../include/gedepth_error.h"
#include <cmath>

#define ERR_THREADS 256
#define ERR_TH 16                                   // tile rows
#define ERR_TW 128                                  // tile columns: 32 groups of four
#define ERR_TG (ERR_TW / 4)
#define ERR_SG (ERR_TG + 2)                         // staged groups per row: the tile's and one halo group on each side (R <= 3 < 4)
#define ERR_SW (4 * ERR_SG)
#define ERR_SR (ERR_TH + 2 * GE_ERROR_MAX_RADIUS)   // staged rows at the largest radius

struct ErrGeom { int Hc, Wc, r0, r1, c0, c1; float scale, lo, hi; };     // as EvalArgs of eval.hip
struct ErrPaint { float tau; int radius, background; };

__constant__ unsigned kErrColour[GE_ERROR_BANDS] = {                      // B | G << 8 | R << 16 of ColorBrewer RdYlBu-10, blue first
    149u | 54u << 8 | 49u << 16,  180u | 117u << 8 | 69u << 16,  209u | 173u << 8 | 116u << 16, 233u | 217u << 8 | 171u << 16,
    248u | 243u << 8 | 224u << 16, 144u | 224u << 8 | 254u << 16, 97u | 174u << 8 | 253u << 16,  67u | 109u << 8 | 244u << 16,
    39u | 48u << 8 | 215u << 16,   38u | 0u << 8 | 165u << 16};

__device__ __forceinline__ int err_band(float n) {
  return (n >= 0.0625f) + (n >= 0.125f) + (n >= 0.25f) + (n >= 0.5f) + (n >= 1.f) + (n >= 2.f) + (n >= 4.f) + (n >= 8.f) + (n >= 16.f);
}

// One group of four ground-truth values at crop position (r, c), c % 4 == 0 or any c with element loads: which of them count, and their e.
// `gs` / `ps`: the group's first ground-truth value / prediction.  PV: one float4 of the prediction (Wc % 4 == 0, 16-byte aligned);
// gv: one 8-byte load of the ground truth.  Element loads touch only columns inside [c0, c1), which lie in the crop.  Returns whether any
// pixel counts; e[k] is set for the counted ones only.
template <bool PV>
__device__ __forceinline__ bool err_group(const float* __restrict__ ps, const uint16_t* __restrict__ gs, bool gv, int r, int c, const ErrGeom& a,
                                          bool take[4], float e[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) take[k] = false;
  if (r < a.r0 || r >= a.r1 || c + 4 <= a.c0 || c >= a.c1) return false;          // nothing of this group is in the rectangle: no loads
  uint16_t raw[4];
  if (PV && gv) {
    const uint2 t = *(const uint2*)gs;
    raw[0] = (uint16_t)t.x; raw[1] = (uint16_t)(t.x >> 16); raw[2] = (uint16_t)t.y; raw[3] = (uint16_t)(t.y >> 16);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = (c + k >= a.c0 && c + k < a.c1) ? gs[k] : (uint16_t)0;
  }
  float gt[4];
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gt[k] = (float)raw[k] / a.scale;
    take[k] = c + k >= a.c0 && c + k < a.c1 && gt[k] > a.lo && gt[k] < a.hi;
    any = any || take[k];
  }
  if (!any) return false;                                                          // no counted pixel: no prediction loads
  float p[4];
  if (PV) {
    const float4 t = *(const float4*)ps;
    p[0] = t.x; p[1] = t.y; p[2] = t.z; p[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = take[k] ? ps[k] : 1.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (take[k]) e[k] = fabsf(gt[k] - p[k]) / gt[k];
  return true;
}

// Four output pixels at crop position (r, c): N[k] < 0 shows the background, else the colour of N[k]'s band.
// ov: three 4-byte stores (out 4-byte aligned, Wc % 4 == 0), else byte stores of the columns below Wc.  `img` starts at the crop's corner.
__device__ __forceinline__ void err_paint(const float N[4], int r, int c, int Wc, const uint8_t* __restrict__ img, int W, int background, bool ov,
                                          uint8_t* __restrict__ out) {
  uint8_t* dst = out + ((long)r * Wc + c) * 3;
  const uint8_t* src = background != 2 ? img + ((long)r * W + c) * 3 : nullptr;
  if (ov && N[0] < 0.f && N[1] < 0.f && N[2] < 0.f && N[3] < 0.f && (background == 2 || ((uintptr_t)src & 3) == 0)) {
    unsigned w0 = 0u, w1 = 0u, w2 = 0u;                                            // twelve background bytes as three words
    if (background != 2) {
      w0 = ((const unsigned*)src)[0]; w1 = ((const unsigned*)src)[1]; w2 = ((const unsigned*)src)[2];
      if (background == 1) { w0 = (w0 >> 1) & 0x7f7f7f7fu; w1 = (w1 >> 1) & 0x7f7f7f7fu; w2 = (w2 >> 1) & 0x7f7f7f7fu; }
    }
    ((unsigned*)dst)[0] = w0; ((unsigned*)dst)[1] = w1; ((unsigned*)dst)[2] = w2;
    return;
  }
  unsigned px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    px[k] = 0u;
    if (c + k >= Wc) continue;
    if (N[k] >= 0.f) {
      px[k] = kErrColour[err_band(N[k])];
    } else if (background != 2) {
      px[k] = (unsigned)src[3 * k] | (unsigned)src[3 * k + 1] << 8 | (unsigned)src[3 * k + 2] << 16;
      if (background == 1) px[k] = (px[k] >> 1) & 0x7f7f7fu;
    }
  }
  if (ov) {
    ((unsigned*)dst)[0] = px[0] | px[1] << 24;
    ((unsigned*)dst)[1] = px[1] >> 8 | px[2] << 16;
    ((unsigned*)dst)[2] = px[2] >> 16 | px[3] << 8;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < Wc) {
        dst[3 * k] = (uint8_t)px[k]; dst[3 * k + 1] = (uint8_t)(px[k] >> 8); dst[3 * k + 2] = (uint8_t)(px[k] >> 16);
      }
  }
}

// four values of the optional err plane at crop position (r, c); ev: one 16-byte store
__device__ __forceinline__ void err_plane_store(float* __restrict__ err, const float e[4], int r, int c, int Wc, bool ev) {
  float* d = err + (long)r * Wc + c;
  if (ev) {
    *(float4*)d = make_float4(e[0], e[1], e[2], e[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < Wc) d[k] = e[k];
  }
}

// Frame f = blockIdx.y of the table (image: the (H, W) uint16 ground truth, aux: the (H, W, 3) uint8 frame or null), tile blockIdx.x.
// pred (n, Hc, Wc), out (n, Hc, Wc, 3), err (n, Hc, Wc) or null.  ov / ev: word stores of out / 16-byte stores of err (uniform).
template <bool PV>
__global__ void __launch_bounds__(ERR_THREADS) error_image_k(const float* __restrict__ pred, BatchTable t, ErrGeom a, ErrPaint ep, bool ov, bool ev,
                                                             uint8_t* __restrict__ out, float* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) float stage[ERR_SR][ERR_SW];           // n of the tile and its halo, -1.f: no source
  __shared__ __attribute__((aligned(16))) float rowmax[ERR_SR][ERR_TW];          // its maximum over |dc| <= R
  const GeBatchFrame fr = t.f[blockIdx.y];
  const int tiles_x = (a.Wc + ERR_TW - 1) / ERR_TW;
  const int ty0 = (int)(blockIdx.x / tiles_x) * ERR_TH, tx0 = (int)(blockIdx.x % tiles_x) * ERR_TW;
  const int R = ep.radius, rows = ERR_TH + 2 * R;
  const long plane = (long)a.Hc * a.Wc, corner = (long)fr.top * fr.W + fr.left;
  const float* p = pred + (long)blockIdx.y * plane;
  uint8_t* o = out + (long)blockIdx.y * plane * 3;
  float* er = err ? err + (long)blockIdx.y * plane : nullptr;
  const uint16_t* gt = (const uint16_t*)fr.image + corner;
  const uint8_t* img = fr.aux ? (const uint8_t*)fr.aux + corner * 3 : nullptr;
  const bool gv = PV && ((uintptr_t)fr.image & 7) == 0 && (fr.W & 3) == 0 && (fr.left & 3) == 0;
  // can a source reach this tile?  (uniform over the workgroup)
  const bool live = a.r0 < a.r1 && a.c0 < a.c1 && ty0 + ERR_TH + R > a.r0 && ty0 - R < a.r1 && tx0 + ERR_TW + R > a.c0 && tx0 - R < a.c1;
  const float none[4] = {-1.f, -1.f, -1.f, -1.f};
  if (live) {
    for (int it = threadIdx.x; it < rows * ERR_SG; it += ERR_THREADS) {
      const int sr = it / ERR_SG, sg = it - sr * ERR_SG;
      const int r = ty0 - R + sr, c = tx0 - 4 + 4 * sg;                            // the rectangle lies in the crop: a group outside the crop takes nothing
      bool take[4];
      float e[4], n[4] = {-1.f, -1.f, -1.f, -1.f}, ee[4] = {-1.f, -1.f, -1.f, -1.f};
      if (err_group<PV>(p + (long)r * a.Wc + c, gt + (long)r * fr.W + c, gv, r, c, a, take, e)) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (take[k]) {
            ee[k] = e[k];
            const float q = e[k] / ep.tau;
            n[k] = q != q ? INFINITY : q;
          }
      }
      *(float4*)&stage[sr][4 * sg] = make_float4(n[0], n[1], n[2], n[3]);
      if (er && sr >= R && sr < R + ERR_TH && sg >= 1 && sg <= ERR_TG && r < a.Hc && c < a.Wc) err_plane_store(er, ee, r, c, a.Wc, ev);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < rows * ERR_TG; it += ERR_THREADS) {            // row pass: output column 4 og + k is staged column 4 og + 4 + k
      const int sr = it / ERR_TG, og = it - sr * ERR_TG;
      float v[12];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float4 q = *(const float4*)&stage[sr][4 * og + 4 * j];
        v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
      }
      float m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        m[k] = v[4 + k];
#pragma unroll
        for (int d = 1; d <= GE_ERROR_MAX_RADIUS; ++d)
          if (d <= R) {
            m[k] = v[4 + k - d] > m[k] ? v[4 + k - d] : m[k];
            m[k] = v[4 + k + d] > m[k] ? v[4 + k + d] : m[k];
          }
      }
      *(float4*)&rowmax[sr][4 * og] = make_float4(m[0], m[1], m[2], m[3]);
    }
    __syncthreads();
  }
  for (int it = threadIdx.x; it < ERR_TH * ERR_TG; it += ERR_THREADS) {             // column pass and paint: four pixels per lane
    const int orow = it / ERR_TG, og = it - orow * ERR_TG;
    const int r = ty0 + orow, c = tx0 + 4 * og;
    if (r >= a.Hc || c >= a.Wc) continue;
    float N[4] = {-1.f, -1.f, -1.f, -1.f};
    if (live) {
      for (int d = 0; d <= 2 * R; ++d) {                                            // staged row orow + R is output row orow
        const float4 q = *(const float4*)&rowmax[orow + d][4 * og];
        N[0] = q.x > N[0] ? q.x : N[0]; N[1] = q.y > N[1] ? q.y : N[1]; N[2] = q.z > N[2] ? q.z : N[2]; N[3] = q.w > N[3] ? q.w : N[3];
      }
    } else if (er) {
      err_plane_store(er, none, r, c, a.Wc, ev);
    }
    err_paint(N, r, c, a.Wc, img, fr.W, ep.background, ov, o);
  }
}

// Thread it owns the four crop pixels of group it and walks the n frames in index order: at each counted pixel with a finite e,
// sum += (double)e, count += 1, in registers from the pixel's first touch, stored once.  pred (n, Hc, Wc).
template <bool PV>
__global__ void __launch_bounds__(ERR_THREADS) error_accumulate_k(const float* __restrict__ pred, BatchTable t, int n, ErrGeom a,
                                                                  double* __restrict__ sum, uint32_t* __restrict__ count) {
  const int G = (a.Wc + 3) >> 2;
  const long it = (long)blockIdx.x * ERR_THREADS + threadIdx.x;
  if (it >= (long)a.Hc * G) return;
  const int r = (int)(it / G), c = 4 * (int)(it - (long)r * G);
  if (r < a.r0 || r >= a.r1 || c + 4 <= a.c0 || c >= a.c1) return;
  const long at = (long)r * a.Wc + c, plane = (long)a.Hc * a.Wc;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  uint32_t cnt[4] = {0u, 0u, 0u, 0u};
  bool touched[4] = {false, false, false, false};
  for (int f = 0; f < n; ++f) {
    const GeBatchFrame fr = t.f[f];
    const uint16_t* gt = (const uint16_t*)fr.image + ((long)fr.top * fr.W + fr.left);
    const bool gv = PV && ((uintptr_t)fr.image & 7) == 0 && (fr.W & 3) == 0 && (fr.left & 3) == 0;
    bool take[4];
    float e[4];
    if (!err_group<PV>(pred + (long)f * plane + at, gt + (long)r * fr.W + c, gv, r, c, a, take, e)) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (take[k] && fabsf(e[k]) < INFINITY) {                                     // NaN and inf enter neither plane
        if (!touched[k]) {
          s[k] = sum[at + k];
          cnt[k] = count[at + k];
          touched[k] = true;
        }
        s[k] += (double)e[k];
        cnt[k] += 1u;
      }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (touched[k]) {
      sum[at + k] = s[k];
      count[at + k] = cnt[k];
    }
}

// what all four entry points refuse, but for their own rule on the prediction's alignment: every bad argument before anything unsupported
static int error_check(const float* pred, const GeBatchFrame* frames, int n, const ErrGeom& a) {
  if (!pred) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, a.Hc, a.Wc, false)) return e;                           // every window lies in its frame
  if (a.r0 < 0 || a.r0 > a.Hc || a.r1 < 0 || a.r1 > a.Hc || a.c0 < 0 || a.c0 > a.Wc || a.c1 < 0 || a.c1 > a.Wc) return GE_ERR_BAD_ARG;
  return GE_OK;
}
static int error_aligned(const GeBatchFrame* frames, int n) {
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].image & 1) return GE_ERR_UNSUPPORTED;
  return GE_OK;
}

static int image_check(const float* pred, const GeBatchFrame* frames, int n, const ErrGeom& a, const ErrPaint& ep, const uint8_t* out,
                       const float* err) {
  if (!out) return GE_ERR_BAD_ARG;
  if (int e = error_check(pred, frames, n, a)) return e;
  if (ep.radius < 0 || ep.radius > GE_ERROR_MAX_RADIUS || ep.background < 0 || ep.background > 2) return GE_ERR_BAD_ARG;
  if (!(ep.tau > 0.f && ep.tau <= 1.f)) return GE_ERR_BAD_ARG;                                       // NaN fails both comparisons
  if (ep.background != 2)
    for (int f = 0; f < n; ++f)
      if (!frames[f].aux) return GE_ERR_BAD_ARG;
  if ((long)((a.Hc + ERR_TH - 1) / ERR_TH) * ((a.Wc + ERR_TW - 1) / ERR_TW) > 0x7fffffffL) return GE_ERR_BAD_ARG;
  if ((uintptr_t)err & 3) return GE_ERR_UNSUPPORTED;
  return error_aligned(frames, n);
}
static int image_launch(const float* pred, const GeBatchFrame* frames, int n, bool pv, const ErrGeom& a, const ErrPaint& ep, uint8_t* out, float* err,
                        void* stream) {
  const dim3 grid((unsigned)(((a.Hc + ERR_TH - 1) / ERR_TH) * ((a.Wc + ERR_TW - 1) / ERR_TW)), (unsigned)n);
  const bool ov = ((uintptr_t)out & 3) == 0 && (a.Wc & 3) == 0, ev = err && ((uintptr_t)err & 15) == 0 && (a.Wc & 3) == 0;
  if (pv)
    error_image_k<true><<<grid, ERR_THREADS, 0, ge_stream(stream)>>>(pred, batch_table(frames, n), a, ep, ov, ev, out, err);
  else
    error_image_k<false><<<grid, ERR_THREADS, 0, ge_stream(stream)>>>(pred, batch_table(frames, n), a, ep, ov, ev, out, err);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" int ge_error_image(const float* pred, const uint16_t* gt_raw, const uint8_t* image, int H, int W, int top, int left, int Hc, int Wc,
                              int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth, float tau, int radius,
                              int background, uint8_t* out, float* err, void* stream) {
  const GeBatchFrame fr = {gt_raw, image, H, W, top, left};
  const ErrGeom a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  const ErrPaint ep = {tau, radius, background};
  if (int e = image_check(pred, &fr, 1, a, ep, out, err)) return e;
  if ((uintptr_t)pred & 3) return GE_ERR_UNSUPPORTED;
  return image_launch(pred, &fr, 1, ((uintptr_t)pred & 15) == 0 && (Wc & 3) == 0, a, ep, out, err, stream);
}

extern "C" int ge_error_image_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                                    float depth_scale, float min_depth, float max_depth, float tau, int radius, int background, uint8_t* out,
                                    float* err, void* stream) {
  const ErrGeom a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  const ErrPaint ep = {tau, radius, background};
  if (int e = image_check(pred, frames, n, a, ep, out, err)) return e;
  if ((Wc & 3) || ((uintptr_t)pred & 15)) return GE_ERR_UNSUPPORTED;
  return image_launch(pred, frames, n, true, a, ep, out, err, stream);
}

static int accumulate_check(const float* pred, const GeBatchFrame* frames, int n, const ErrGeom& a, const double* sum, const uint32_t* count) {
  if (!sum || !count) return GE_ERR_BAD_ARG;
  if (int e = error_check(pred, frames, n, a)) return e;
  if (((uintptr_t)sum & 7) || ((uintptr_t)count & 3)) return GE_ERR_UNSUPPORTED;
  return error_aligned(frames, n);
}
static int accumulate_launch(const float* pred, const GeBatchFrame* frames, int n, bool pv, const ErrGeom& a, double* sum, uint32_t* count,
                             void* stream) {
  const unsigned blocks = ge_blocks((long)a.Hc * ((a.Wc + 3) >> 2), ERR_THREADS, 0x7fffffffL);
  if (pv)
    error_accumulate_k<true><<<blocks, ERR_THREADS, 0, ge_stream(stream)>>>(pred, batch_table(frames, n), n, a, sum, count);
  else
    error_accumulate_k<false><<<blocks, ERR_THREADS, 0, ge_stream(stream)>>>(pred, batch_table(frames, n), n, a, sum, count);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" int ge_error_accumulate(const float* pred, const uint16_t* gt_raw, int H, int W, int top, int left, int Hc, int Wc, int r0, int r1,
                                   int c0, int c1, float depth_scale, float min_depth, float max_depth, double* sum, uint32_t* count,
                                   void* stream) {
  const GeBatchFrame fr = {gt_raw, nullptr, H, W, top, left};
  const ErrGeom a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  if (int e = accumulate_check(pred, &fr, 1, a, sum, count)) return e;
  if ((uintptr_t)pred & 3) return GE_ERR_UNSUPPORTED;
  return accumulate_launch(pred, &fr, 1, ((uintptr_t)pred & 15) == 0 && (Wc & 3) == 0, a, sum, count, stream);
}

extern "C" int ge_error_accumulate_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                                         float depth_scale, float min_depth, float max_depth, double* sum, uint32_t* count, void* stream) {
  const ErrGeom a = {Hc, Wc, r0, r1, c0, c1, depth_scale, min_depth, max_depth};
  if (int e = accumulate_check(pred, frames, n, a, sum, count)) return e;
  if ((Wc & 3) || ((uintptr_t)pred & 15)) return GE_ERR_UNSUPPORTED;
  return accumulate_launch(pred, frames, n, true, a, sum, count, stream);
}
