/*
 * gedepth_sweep.h — C ABI of the prior sweep's front end of libgedepth_hip.so (csrc/infer.hip): one KITTI frame into n slots of the
 * batched engine's input that differ only in their two ground channels.
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Declared here and not in an existing header: those do not
 * change with it.
 *
 * THE PERTURBATION RULE.  A variant (c, s, drop) maps a raw ground depth pe (f32) to pe' (f32), all arithmetic in f32, no contraction:
 *
 *     drop                         : pe' = 0
 *     c == 0 and s == 1            : pe' = pe                     the baseline: the plane passes through untouched, bit for bit
 *     not (pe > 0)  (0, < 0, NaN)  : pe' = pe
 *     otherwise                    : q = 1.f / pe + c;   pe' = q > 0.f ? s / q : 0.f
 *
 * c = tan(pitch) / camera height, formed in double by the host and rounded once; s = the height scale.  It is the model's own slope
 * convention (ge_slope_class: slope = atan(h / gt - h / pe); ground_pixel of csrc/ground.hip): a ground truth on a road that rises by
 * `pitch` sits at pe'.  pitch > 0 brings the ground closer, as when the camera pitches down against its calibration; s is the plane of
 * a camera s times as high.  1 / (1 / pe) is not pe in f32, hence the baseline's branch of its own.
 */
#ifndef GEDEPTH_SWEEP_H
#define GEDEPTH_SWEEP_H

#include <stddef.h>
#include <stdint.h>

#include "gedepth_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float c, s; int drop; } GePriorVariant;
#define GE_SWEEP_MAX GE_BATCH_MAX

size_t ge_prior_variant_size(void);   /* sizeof(GePriorVariant), for a binding to check its mirror of the struct against */

/*
 * ge_infer_front_sweep: ONE launch.  The (Hc, Wc) window at (top, left) of the (H, W, 3) uint8 BGR frame and of its raw (H, W) f32
 * ground depth `pe` is read once; images views * v .. views * v + views - 1 of dst (views * n, 5, Hc, Wc) planar f32 carry exactly the
 * bits ge_infer_front writes for the same frame when it is given the plane pe'_v of the rule above (channel 3: pe'_v zeroed above
 * pe_max or below 0 and divided by depth_scale where positive; channel 4: pe'_v itself).  Nothing beyond image views * n is written.
 * `variants` is a HOST array of n entries, read during the call: they travel by value in the kernel-argument block (8 x 12 = 96 bytes)
 * and the array may be reused as soon as the call returns.
 * GE_ERR_BAD_ARG: a null pointer (bgr_hwc, pe, variants, dst, mean3, std3), n outside 1 .. GE_SWEEP_MAX, a non-positive size, a window
 * outside (H, W), views outside 1 .. 2, a variant with a non-finite c or with s non-finite or <= 0.  GE_ERR_UNSUPPORTED: Wc % 4 != 0,
 * dst not 16-byte aligned, pe not 4-byte aligned.
 */
int ge_infer_front_sweep(const uint8_t* bgr_hwc, const float* pe, int H, int W, int top, int left, const GePriorVariant* variants, int n,
                         float* dst, int Hc, int Wc, int views, float pe_max, const double* mean3, const double* std3, float depth_scale,
                         int to_rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_SWEEP_H */
