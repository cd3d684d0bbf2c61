/*
 * gedepth_eval.h — C ABI of the evaluation entry points of libgedepth_hip.so (csrc/eval.hip).
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  These entry points are declared here and not in
 * gedepth_hip.h: that header is the training / inference ABI whose version ge_abi_version() reports, and it does not change with them.
 */
#ifndef GEDEPTH_EVAL_H
#define GEDEPTH_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ge_depth_metrics: the masked metric sums of the KITTI evaluation protocol for one image (depth/core/evaluation/metrics.py:8-100 behind
 * depth/datasets/kitti.py:502-552: KB crop of the ground truth, Garg / Eigen rectangle, min / max depth mask).
 *
 *   pred      (Hc, Wc) f32, the prediction;
 *   gt_raw    (H, W) uint16, the undivided ground-truth PNG; gt = (float)raw / depth_scale (IEEE f32 division), read in the window that
 *             starts at (top, left);
 *   a pixel counts when gt > min_depth && gt < max_depth (f32 comparisons) and it lies in rows [r0, r1) x columns [c0, c1) of the crop
 *   (0 <= r0, r1 <= Hc and 0 <= c0, c1 <= Wc; r0 >= r1 or c0 >= c1 is an empty rectangle: n = 0);
 *   sums[0..9] (f64): n, #(ratio < 1.25), #(ratio < 1.25^2), #(ratio < 1.25^3), sum |d| / gt, sum d^2 / gt, sum d^2, sum l, sum l^2,
 *             sum |log10 gt - log10 pred|, with ratio = max(gt / pred, pred / gt) in f32 (NaN-propagating, as numpy.maximum),
 *             d = gt - pred and l = log pred - log gt in f64 from the two f32 values;
 *   partials  ge_depth_metrics_workspace(Hc, Wc) bytes, 8-byte aligned: ten f64 per workgroup of the first pass.  A second, single
 *             workgroup adds them in index order: no atomics, the same bits on every run.
 * GE_ERR_BAD_ARG: a null pointer, a non-positive size, a window outside (H, W) or a rectangle outside the crop.
 */
int ge_depth_metrics(const float* pred, const uint16_t* gt_raw, int H, int W, int top, int left, int Hc, int Wc,
                     int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth,
                     double* partials, double* sums, void* stream);
size_t ge_depth_metrics_workspace(int Hc, int Wc);   /* bytes of `partials`; 0 for non-positive sizes */

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_EVAL_H */
