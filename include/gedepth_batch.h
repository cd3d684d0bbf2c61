/*
 * gedepth_batch.h — C ABI of the batched KITTI inference / evaluation entry points of libgedepth_hip.so (csrc/infer.hip: front end and
 * merge; csrc/eval.hip: metric sums).
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Declared here and not in gedepth_hip.h: that header is the
 * versioned training / inference ABI, and it does not change with these.
 *
 * Each entry point is ONE launch (the metric sums: two) for n <= GE_BATCH_MAX frames, the frame index on blockIdx.y.  The frames' pointers
 * and geometry are read from the HOST array `frames` during the call and travel by value in the kernel-argument struct (8 x 32 = 256
 * bytes): there is no device-side table, no extra copy, and the array may be reused as soon as the call returns.  The single-frame entry
 * points (ge_infer_front, ge_tta_merge, ge_depth_metrics) launch these very kernels with n = 1 and the same grid.x, so a frame has the same
 * bits from either; what pins the bits is independent of both: the training pipeline's chain ge_aug_load -> ge_aug_color_normalize ->
 * ge_aug_window for the front end, the expression (a + mirror(b)) / 2 for the merge, float64 sums for the metrics (tests/).
 */
#ifndef GEDEPTH_BATCH_H
#define GEDEPTH_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GE_BATCH_MAX 8

/*
 * One frame of a batch.  ge_infer_front_batch: `image` the (H, W, 3) uint8 BGR frame, `aux` its raw (H, W) f32 ground depth.
 * ge_depth_metrics_batch: `image` the (H, W) uint16 ground-truth PNG, `aux` unused (may be null).  (top, left): where the (Hc, Wc) crop
 * window starts in the frame.
 */
typedef struct GeBatchFrame {
  const void* image;
  const void* aux;
  int H, W, top, left;
} GeBatchFrame;

size_t ge_batch_frame_size(void);   /* sizeof(GeBatchFrame), for a binding to check its mirror of the struct against */

/*
 * ge_infer_front_batch: ge_infer_front for n frames that may differ in size and crop offsets.  dst (views * n, 5, Hc, Wc) planar f32,
 * frame-major: view v of frame f is image views * f + v (n = 1: the layout of ge_infer_front).  Nothing beyond image views * n is written.
 * GE_ERR_BAD_ARG: a null pointer (frames, an image, an aux, dst, mean3, std3), n outside 1 .. GE_BATCH_MAX, a non-positive size, views
 * outside 1 .. 2 or a window that leaves its frame.  GE_ERR_UNSUPPORTED: Wc % 4 != 0, dst not 16-byte aligned, an aux not 4-byte aligned.
 */
int ge_infer_front_batch(const GeBatchFrame* frames, int n, float* dst, int Hc, int Wc, int views, float pe_max, const double* mean3,
                         const double* std3, float depth_scale, int to_rgb, void* stream);

/*
 * ge_tta_merge_batch: ge_tta_merge for n frames.  src (2 n, H, W) f32, frame-major as ge_infer_front_batch writes the views;
 * dst (n, H, W) f32 = (src[2 f] + mirror(src[2 f + 1])) / 2.  GE_ERR_BAD_ARG: a null pointer, n outside 1 .. GE_BATCH_MAX, a non-positive
 * size.  GE_ERR_UNSUPPORTED: W % 4 != 0, src or dst not 16-byte aligned.
 */
int ge_tta_merge_batch(const float* src, float* dst, int n, int H, int W, void* stream);

/*
 * ge_depth_metrics_batch: ge_depth_metrics (gedepth_eval.h) for n images.  pred (n, Hc, Wc) f32; frames[f].image the (H, W) uint16 ground
 * truth of image f, read in the window at (top, left); the rectangle and the three depth parameters are shared.  sums (n, 10) f64, row f
 * the ten sums of image f with the bits ge_depth_metrics gives for it (the same kernels): the first pass runs one block partition (it depends
 * on (Hc, Wc) only) once per image on grid.y, the second folds each image's partials in index order on grid.x = n; no atomics.  Whether an
 * image's ground truth is read with 8-byte loads (W % 4 == 0, left % 4 == 0, base 8-byte aligned) is decided per image.
 *   partials  ge_depth_metrics_batch_workspace(n, Hc, Wc) bytes, 8-byte aligned.
 * GE_ERR_BAD_ARG: a null pointer (pred, frames, an image, partials, sums), n outside 1 .. GE_BATCH_MAX, a non-positive size, a window
 * outside its frame or a rectangle outside the crop.  GE_ERR_UNSUPPORTED: Wc % 4 != 0, pred not 16-byte aligned, an image not 2-byte
 * aligned, partials or sums not 8-byte aligned.
 */
int ge_depth_metrics_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                           float depth_scale, float min_depth, float max_depth, double* partials, double* sums, void* stream);
size_t ge_depth_metrics_batch_workspace(int n, int Hc, int Wc);   /* bytes of `partials`; 0 for n outside 1 .. GE_BATCH_MAX or non-positive sizes */

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_BATCH_H */
