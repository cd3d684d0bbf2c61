// Batched KITTI inference and evaluation (include/gedepth_batch.h; gedepth_amd/depth/apis/batch_inference.py): the front end, the flip-TTA
// merge and the metric sums of up to GE_BATCH_MAX = 8 frames per launch, the frame index on blockIdx.y.
//
// The frames of a batch differ in size (the KITTI days are 375 x 1242, 370 x 1224, 374 x 1238, 376 x 1241), crop offsets and ground depth,
// so each has its own pointers and geometry.  They travel BY VALUE in the kernel-argument struct: BatchTable is 8 x 32 = 256 bytes of the
// kernarg segment, which the host fills from the caller's array at launch.  A workgroup reads its frame's entry with scalar loads at a
// uniform offset; there is no device-side pointer table to keep alive and no host-to-device copy ordered before the launch.
//
// Per frame the work is that of the single-frame kernels, through the same device functions (common.h: ge_infer_front_group,
// ge_tta_merge_group; eval_sums.h: metrics_window_sums, metrics_block_fold) over the same grid.x, so every frame gets the bits of
// ge_infer_front / ge_tta_merge / ge_depth_metrics.  Streaming work sized by launch latency: one launch instead of n.
#pragma clang fp contract(off)
#include "eval_sums.h"
#include "../../include/gedepth_batch.h"

struct BatchTable { GeBatchFrame f[GE_BATCH_MAX]; };
static_assert(sizeof(GeBatchFrame) == 32 && sizeof(BatchTable) == 256, "the by-value frame table is 8 x {two pointers, four ints}");

extern "C" size_t ge_batch_frame_size(void) { return sizeof(GeBatchFrame); }

// 0, or the error of a frame list: null list / n outside 1 .. GE_BATCH_MAX / a null image / (need_aux) a null aux / a window outside its frame
static int batch_frames_check(const GeBatchFrame* frames, int n, int Hc, int Wc, bool need_aux) {
  if (!frames || n < 1 || n > GE_BATCH_MAX || Hc <= 0 || Wc <= 0) return GE_ERR_BAD_ARG;
  for (int f = 0; f < n; ++f) {
    const GeBatchFrame& fr = frames[f];
    if (!fr.image || (need_aux && !fr.aux) || fr.H <= 0 || fr.W <= 0 || fr.top < 0 || fr.left < 0) return GE_ERR_BAD_ARG;
    if (Hc > fr.H - fr.top || Wc > fr.W - fr.left) return GE_ERR_BAD_ARG;
  }
  return GE_OK;
}
static BatchTable batch_table(const GeBatchFrame* frames, int n) {
  BatchTable t;
  for (int f = 0; f < GE_BATCH_MAX; ++f) t.f[f] = frames[f < n ? f : 0];     // entries >= n are never read (grid.y = n)
  return t;
}

// dst (views * n, 5, Hc, Wc); frame f = blockIdx.y owns images views * f .. views * f + views - 1.
__global__ void __launch_bounds__(256) infer_front_batch_k(BatchTable t, float* __restrict__ dst, int Hc, int Wc, int views, InferNorm p) {
  const GeBatchFrame fr = t.f[blockIdx.y];
  const int G = Wc >> 2;
  const long n = (long)Hc * Wc, groups = (long)Hc * G;
  float* out = dst + (long)blockIdx.y * views * 5 * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256)
    ge_infer_front_group((const uint8_t*)fr.image, (const float*)fr.aux, out, fr.W, fr.top, fr.left, Wc, views, p, i, G, n);
}
extern "C" int ge_infer_front_batch(const GeBatchFrame* frames, int n, float* dst, int Hc, int Wc, int views, float pe_max,
                                    const double* mean3, const double* std3, float depth_scale, int to_rgb, void* stream) {
  if (!dst || !mean3 || !std3 || (views != 1 && views != 2)) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, Hc, Wc, true)) return e;
  if ((Wc & 3) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].aux & 3) return GE_ERR_UNSUPPORTED;
  InferNorm p;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.stdinv[c] = 1.0 / std3[c]; }
  p.pe_max = pe_max; p.depth_scale = depth_scale; p.to_rgb = to_rgb;
  const long groups = (long)Hc * (Wc / 4);
  const dim3 grid(ge_blocks(groups, 256, 65536), (unsigned)n);                // grid.x: that of ge_infer_front
  infer_front_batch_k<<<grid, 256, 0, ge_stream(stream)>>>(batch_table(frames, n), dst, Hc, Wc, views, p);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

// src (2 n, H, W), dst (n, H, W); frame f = blockIdx.y.
__global__ void __launch_bounds__(256) tta_merge_batch_k(const float* __restrict__ src, float* __restrict__ dst, int H, int W) {
  const int G = W >> 2;
  const long n = (long)H * W, groups = (long)H * G;
  const float* s = src + (long)blockIdx.y * 2 * n;
  float* d = dst + (long)blockIdx.y * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) ge_tta_merge_group(s, d, W, i, G, n);
}
extern "C" int ge_tta_merge_batch(const float* src, float* dst, int n, int H, int W, void* stream) {
  if (!src || !dst || n < 1 || n > GE_BATCH_MAX || H <= 0 || W <= 0) return GE_ERR_BAD_ARG;
  if ((W & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return GE_ERR_UNSUPPORTED;
  const dim3 grid(ge_blocks((long)H * (W / 4), 256, 65536), (unsigned)n);
  tta_merge_batch_k<<<grid, 256, 0, ge_stream(stream)>>>(src, dst, H, W);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

// Metric sums.  pred (n, Hc, Wc), 16-byte aligned with Wc % 4 == 0, so every image's prediction takes the float4 loads (PV of eval_sums.h);
// the ground truth's 8-byte loads (GV) are a per-image choice, uniform over the workgroup.  partials (n, gridDim.x, 10).
struct BatchEvalArgs { int Hc, Wc, r0, r1, c0, c1; float scale, lo, hi; };
__global__ void __launch_bounds__(GE_EVAL_THREADS) metrics_partial_batch_k(const float* __restrict__ pred, BatchTable t, BatchEvalArgs b,
                                                                           double* __restrict__ partials) {
  __shared__ double red[GE_EVAL_THREADS / GE_WAVE][GE_EVAL_SUMS];
  const GeBatchFrame fr = t.f[blockIdx.y];
  EvalArgs a;
  a.W = fr.W; a.top = fr.top; a.left = fr.left; a.Hc = b.Hc; a.Wc = b.Wc; a.r0 = b.r0; a.r1 = b.r1; a.c0 = b.c0; a.c1 = b.c1;
  a.scale = b.scale; a.lo = b.lo; a.hi = b.hi;
  double acc[GE_EVAL_SUMS];
#pragma unroll
  for (int k = 0; k < GE_EVAL_SUMS; ++k) acc[k] = 0.0;
  const float* p = pred + (long)blockIdx.y * b.Hc * b.Wc;
  const uint16_t* gt = (const uint16_t*)fr.image;
  if (((uintptr_t)gt & 7) == 0 && (fr.W & 3) == 0 && (fr.left & 3) == 0)      // ge_depth_metrics' `gv`
    metrics_window_sums<true, true>(p, gt, a, acc);
  else
    metrics_window_sums<true, false>(p, gt, a, acc);
  metrics_block_fold(acc, red, partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * GE_EVAL_SUMS);
}
// image f = blockIdx.x: its partials in index order, as metrics_fold_k of eval.hip adds them
__global__ void __launch_bounds__(GE_WAVE) metrics_fold_batch_k(const double* __restrict__ partials, int blocks, double* __restrict__ sums) {
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

extern "C" int ge_depth_metrics_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                                      float depth_scale, float min_depth, float max_depth, double* partials, double* sums, void* stream) {
  if (!pred || !partials || !sums) return GE_ERR_BAD_ARG;
  if (int e = batch_frames_check(frames, n, Hc, Wc, false)) return e;
  if (r0 < 0 || r0 > Hc || r1 < 0 || r1 > Hc || c0 < 0 || c0 > Wc || c1 < 0 || c1 > Wc) return GE_ERR_BAD_ARG;
  if ((Wc & 3) || ((uintptr_t)pred & 15) || ((uintptr_t)partials & 7) || ((uintptr_t)sums & 7)) return GE_ERR_UNSUPPORTED;
  for (int f = 0; f < n; ++f)
    if ((uintptr_t)frames[f].image & 1) return GE_ERR_UNSUPPORTED;
  hipStream_t s = ge_stream(stream);
  BatchEvalArgs b;
  b.Hc = Hc; b.Wc = Wc; b.r0 = r0; b.r1 = r1; b.c0 = c0; b.c1 = c1; b.scale = depth_scale; b.lo = min_depth; b.hi = max_depth;
  const unsigned blocks = metrics_blocks(Hc, Wc);                             // ge_depth_metrics' partition
  metrics_partial_batch_k<<<dim3(blocks, (unsigned)n), GE_EVAL_THREADS, 0, s>>>(pred, batch_table(frames, n), b, partials);
  GE_LAUNCH_CHECK();
  metrics_fold_batch_k<<<(unsigned)n, GE_WAVE, 0, s>>>(partials, (int)blocks, sums);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
