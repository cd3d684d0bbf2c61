/*
 * gedepth_strata.h — C ABI of the stratified KITTI metric sums of libgedepth_hip.so (csrc/eval.hip): the ten sums of ge_depth_metrics
 * (gedepth_eval.h) per distance bin and per on / off ground class of the ground truth.
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Declared here and not in gedepth_hip.h: that header is the
 * versioned training / inference ABI, and it does not change with these.
 *
 * Every pixel that ge_depth_metrics counts (inside the rectangle, min_depth < gt < max_depth) falls into exactly one of S = B * C <= 16
 * strata.  All arithmetic is f32 with `fp contract(off)`:
 *
 *   distance bin   edges[0 .. B-2] are finite and strictly ascending, B = n_edges + 1, 1 <= B <= 8.
 *                  bin = #{ j : gt >= edges[j] }, with gt = (float)raw / depth_scale as in ge_depth_metrics.  A ground truth exactly on an
 *                  edge belongs to the upper bin.  Edges outside (min_depth, max_depth) are allowed and simply leave bins empty.
 *   ground class   C = 2 when a ground-depth plane is given, else C = 1.  g is the frame's raw (H, W) f32 ground depth, read at the same
 *                  (top + r, left + c) as the ground truth.
 *                  on_ground = g > 0.f && fabsf(gt - g) <= ground_tol * g.  A NaN g is off the ground.  On a flat road this reads "the
 *                  return lies within ground_tol * cam_height of the plane".  ground_tol is a caller's parameter in [0, 1] (0.1 is the
 *                  Python layers' default); it is not a measured constant.
 *   stratum = bin * C + on_ground.
 *
 * Row s of the result carries, bit for bit, the ten doubles that ge_depth_metrics gives for the same pred when the ground truth of every
 * pixel outside stratum s is set to 0 (min_depth >= 0): the stratum is on blockIdx.z of ge_depth_metrics' first pass, a workgroup of
 * stratum s walks the crop as that pass does and adds only the pixels of s, and the fold adds each (image, stratum) row's partials in index
 * order.  No atomics, the same bits on every run; with n_edges = 0 and no ground plane the one row is ge_depth_metrics' row.
 */
#ifndef GEDEPTH_STRATA_H
#define GEDEPTH_STRATA_H

#include <stddef.h>
#include <stdint.h>

#include "gedepth_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GE_STRATA_MAX_EDGES 7
#define GE_STRATA_MAX 16

int ge_depth_strata_count(int n_edges, int use_ground);   /* S = (n_edges + 1) * (use_ground ? 2 : 1), or 0 for n_edges outside 0 .. 7 */

/* bytes of `partials` = n * strata * ge_depth_metrics_workspace(Hc, Wc); 0 for n outside 1 .. GE_BATCH_MAX, strata outside 1 .. 16 or non-positive sizes */
size_t ge_depth_metrics_strata_workspace(int n, int Hc, int Wc, int strata);

/*
 * ge_depth_metrics_strata: one image.  pred, gt_raw, the window, the rectangle and the three depth parameters as in ge_depth_metrics.
 *   ground    (H, W) f32 or null (C = 1), 4-byte aligned; read with 16-byte loads where pred is (16-byte aligned, Wc % 4 == 0) and
 *             W % 4 == 0, left % 4 == 0 and its base is 16-byte aligned, and only for groups with a counted pixel;
 *   edges     n_edges floats on the HOST, read during the call; may be null when n_edges == 0;
 *   partials  ge_depth_metrics_strata_workspace(1, Hc, Wc, S) bytes, 8-byte aligned;
 *   sums      (S, 10) f64, row s as stated above.
 * GE_ERR_BAD_ARG: a null pointer, a non-positive size, a window outside (H, W), a rectangle outside the crop, n_edges outside 0 .. 7, edges
 * that are not finite and strictly ascending, a ground_tol that is NaN, negative or above 1.  GE_ERR_UNSUPPORTED: pred or ground not
 * 4-byte aligned, gt_raw not 2-byte aligned, partials or sums not 8-byte aligned.  Every check comes before a launch.
 */
int ge_depth_metrics_strata(const float* pred, const uint16_t* gt_raw, const float* ground, int H, int W, int top, int left, int Hc, int Wc,
                            int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth, const float* edges, int n_edges,
                            float ground_tol, double* partials, double* sums, void* stream);

/*
 * ge_depth_metrics_strata_batch: the same kernels for n images, as ge_depth_metrics_batch is to ge_depth_metrics.  pred (n, Hc, Wc) f32;
 * frames[f].image the ground truth of image f and frames[f].aux its ground plane: all null (C = 1) or none null (C = 2).
 * sums (n, S, 10) f64, block f with the bits ge_depth_metrics_strata gives for image f; partials
 * ge_depth_metrics_strata_workspace(n, Hc, Wc, S) bytes.
 * GE_ERR_BAD_ARG as above, and n outside 1 .. GE_BATCH_MAX or an aux that is null for some frames and set for others.
 * GE_ERR_UNSUPPORTED as above, and Wc % 4 != 0 or pred not 16-byte aligned.
 */
int ge_depth_metrics_strata_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                                  float depth_scale, float min_depth, float max_depth, const float* edges, int n_edges, float ground_tol,
                                  double* partials, double* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_STRATA_H */
