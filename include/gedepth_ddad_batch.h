/*
 * gedepth_ddad_batch.h — C ABI of the batched DDAD test-protocol entry points of libgedepth_hip.so (csrc/infer.hip: front end;
 * csrc/eval.hip: resized metric sums).
 *
 * Same conventions as gedepth_ddad.h (extern "C", 0 on success, GE_ERR_* of gedepth_hip.h for argument errors, every GE_ERR_BAD_ARG before
 * any GE_ERR_UNSUPPORTED, device pointers owned by the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Declared here
 * and not in gedepth_ddad.h or gedepth_batch.h: those headers do not change with these entry points.
 *
 * As in gedepth_batch.h, whose GeBatchFrame and GE_BATCH_MAX these entry points reuse: n <= GE_BATCH_MAX frames per launch, the frame
 * index on blockIdx.y, the frames' pointers and sizes read from the HOST array `frames` during the call and carried by value in the
 * kernel-argument struct.  The single-frame entry points of gedepth_ddad.h launch these very kernels with n = 1 and the same grid.x, so a
 * frame has the same bits from either.
 */
#ifndef GEDEPTH_DDAD_BATCH_H
#define GEDEPTH_DDAD_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gedepth_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ge_infer_front_ddad_batch: ge_infer_front_ddad for n frames that may differ in size and ground depth (the cameras of one batch).
 * frames[f]: `image` the (H, W, 3) uint8 BGR frame, `aux` that camera's raw (H, W) f32 ground depth, H and W its own, top = left = 0
 * (DDADResize takes the whole frame).  dst (n, 5, Hd, Wd) planar f32, image f the frame f as ge_infer_front_ddad writes it; nothing beyond
 * image n is written.  One launch.
 * GE_ERR_BAD_ARG: a null pointer (frames, an image, an aux, dst, mean3, std3), n outside 1 .. GE_BATCH_MAX, a non-positive size, a
 * non-zero top or left.  GE_ERR_UNSUPPORTED: Hd > H or Wd > W of a frame (the area filter only shrinks), Wd % 4 != 0, dst not 16-byte
 * aligned, an aux not 4-byte aligned.
 */
int ge_infer_front_ddad_batch(const GeBatchFrame* frames, int n, float* dst, int Hd, int Wd, float pe_max, const double* mean3,
                              const double* std3, float depth_scale, int to_rgb, void* stream);

/*
 * ge_depth_metrics_resized_batch: ge_depth_metrics_resized for n images.  pred (n, h, w) f32; frames[f].image the (H, W) f32 ground truth
 * of image f in metres (`aux` unused, may be null; top = left = 0).  All n ground truths have ONE size (H, W): the block partition of the
 * first pass depends on it alone and is the single-frame call's, run once per image on grid.y; the second pass folds each image's
 * partials in index order on grid.x = n.  sums (n, 10) f64, row f the ten sums of image f with the bits ge_depth_metrics_resized gives for
 * it (the same kernels); no atomics, the same bits on every run.  Whether an image's ground truth is read with 16-byte loads (its base
 * 16-byte aligned, W % 4 == 0) is decided per image.
 *   partials  ge_depth_metrics_resized_batch_workspace(n, H, W) bytes, 8-byte aligned.
 * GE_ERR_BAD_ARG: a null pointer (pred, frames, an image, partials, sums), n outside 1 .. GE_BATCH_MAX, a non-positive size, a non-zero top
 * or left.  GE_ERR_UNSUPPORTED: ground truths of more than one size, pred or an image not 4-byte aligned, partials or sums not 8-byte
 * aligned.
 */
int ge_depth_metrics_resized_batch(const float* pred, int h, int w, const GeBatchFrame* frames, int n, float min_depth, float max_depth,
                                   double* partials, double* sums, void* stream);
size_t ge_depth_metrics_resized_batch_workspace(int n, int H, int W);   /* bytes of `partials`; 0 for n outside 1 .. GE_BATCH_MAX or non-positive sizes */

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_DDAD_BATCH_H */
