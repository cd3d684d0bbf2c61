/*
 * gedepth_ddad.h — C ABI of the DDAD test-protocol entry points of libgedepth_hip.so (csrc/infer.hip, csrc/eval.hip).
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Like gedepth_eval.h, this header stands beside the versioned
 * training / inference ABI of gedepth_hip.h and beside the KITTI evaluation ABI of gedepth_eval.h: neither changes with these entry points.
 */
#ifndef GEDEPTH_DDAD_H
#define GEDEPTH_DDAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ge_infer_front_ddad: the per-frame front end of the DDAD test pipeline, LoadDDADImageFromFile(USEPE, USE_DYNAMIC_PE) ->
 * DDADResize(shape, depth = False) -> Normalize, in one launch.
 *
 *   bgr_hwc   (H, W, 3) uint8, the frame;      pe  (H, W) f32, the camera's raw ground depth;
 *   dst       (1, 5, Hd, Wd) planar f32, 16-byte aligned, Wd % 4 == 0 (else GE_ERR_UNSUPPORTED; so is Hd > H or Wd > W: the area filter
 *             only shrinks);
 *   channels 0-2: the frame area-averaged to (Hd, Wd) (float64 weights, rint, clamp: ge_aug_area_u8), then BGR -> RGB when to_rgb and
 *             (x - mean) * (1 / std) in float64 rounded to f32 (mean3 / std3: three host doubles in output channel order);
 *   channel 3: nearest-neighbour pe (source index min(floor(dst * in / out), in - 1) in float64: ge_aug_resize mode 0), values > pe_max or
 *             < 0 zeroed, positive ones divided by depth_scale;     channel 4: nearest-neighbour raw pe.
 */
int ge_infer_front_ddad(const uint8_t* bgr_hwc, const float* pe, float* dst, int H, int W, int Hd, int Wd, float pe_max,
                        const double* mean3, const double* std3, float depth_scale, int to_rgb, void* stream);

/*
 * ge_depth_metrics_resized: the ten metric sums of ge_depth_metrics (gedepth_eval.h) for the DDAD evaluation protocol
 * (depth/datasets/ddad.py pre_eval): the prediction is resized bilinearly, align_corners = True, to the ground truth, and every pixel with
 * gt > min_depth && gt < max_depth (f32 comparisons) counts; there is no crop rectangle.  The resized map is never stored.
 *
 *   pred  (h, w) f32;      gt  (H, W) f32, metres (the .npz's `depth` array as it is);
 *   for a counted pixel (Y, X), in f32 without contraction: scale = (float)(h - 1) / (float)(H - 1) (0 when H == 1), src = scale * (float)Y,
 *   i0 = (int)src, i1 = min(i0 + 1, h - 1), w1 = src - (float)i0, w0 = 1.f - w1, the same in x, and
 *   p = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);  p and gt then enter the sums as in ge_depth_metrics;
 *   partials  ge_depth_metrics_resized_workspace(H, W) bytes, 8-byte aligned; no atomics, the same bits on every run.
 * GE_ERR_BAD_ARG: a null pointer or a non-positive size.  GE_ERR_UNSUPPORTED: pred / gt not 4-byte, partials / sums not 8-byte aligned.
 */
int ge_depth_metrics_resized(const float* pred, int h, int w, const float* gt, int H, int W, float min_depth, float max_depth,
                             double* partials, double* sums, void* stream);
size_t ge_depth_metrics_resized_workspace(int H, int W);   /* bytes of `partials`; 0 for non-positive sizes */

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_DDAD_H */
