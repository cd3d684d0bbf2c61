/*
 * gedepth_ground.h — C ABI of the ground-map entry point of libgedepth_hip.so (csrc/ground.hip).
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Like gedepth_eval.h, gedepth_ddad.h and gedepth_cloud.h, this
 * header stands beside the versioned training / inference ABI of gedepth_hip.h, which does not change with this entry point.
 */
#ifndef GEDEPTH_GROUND_H
#define GEDEPTH_GROUND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ge_ground_maps: the ground embedding's own maps at image resolution, merged over the V (1 or 2) views of one inference frame, from
 * the low-resolution outputs of the two ground necks.  One launch; the 11 up-sampled slope logits are never written.
 *
 *   logits_lr    (V, 11, h, w) f32 slope logits, or NULL for the vanilla model;
 *   y_lr         (V, 1, h, w) f32 ground attention;
 *   pe           view v's (H, W) f32 ground plane at pe + v * pe_bs (elements): the RAW ground depth for the adaptive model, the
 *                NORMALISED one (depth / scale, 0 where invalid) for the vanilla model;
 *   height       NULL (1.65 m) or V f32 camera heights on the device (adaptive model only);
 *   depth_scale  the adaptive model's validity bound; gain: the vanilla model's factor (200);
 *   flip         non-zero: view 1 is the horizontal mirror of the frame, so output column X reads view 1 at column W - 1 - X.
 *
 * Per view v at its own pixel, with both low-resolution operands up-sampled bilinearly (align_corners = False) exactly as
 * ge_ground_embed_fwd / ge_ground_vanilla_fwd up-sample them:
 *   adaptive     deg_v = sum_c softmax(logits)_c (c - 5), off_v = -height / ((-height / (pe + 1e-8) - tan(deg_v pi / 180)) + 1e-8),
 *                m_v = 1 where 0 < off_v <= depth_scale else 0, t_v = (off_v m_v) y_v (the pe_mask of ge_ground_embed_fwd, bit for bit),
 *                ok_v = (m_v == 1);
 *   vanilla      t_v = pe y_v gain (the pe_mask of ge_ground_vanilla_fwd), off_v = pe gain, ok_v = pe > 0, deg_v = 0.
 * Outputs:
 *   maps         (4, H, W) f32, 4-byte aligned:
 *                  plane 0  attention     (y_0 + y_1) * 0.5f                                  V = 1: y_0
 *                  plane 1  ground_term   (t_0 + t_1) * 0.5f  (NaN propagates)               V = 1: t_0
 *                  plane 2  ground_depth  the mean of off_v over the views with ok_v: (off_0 + off_1) * 0.5f, the single valid one,
 *                                         or 0 when no view is valid
 *                  plane 3  slope_deg     (deg_0 + deg_1) * 0.5f                              V = 1: deg_0; all zeros for vanilla
 *   valid        (H, W) uint8: the number of views with ok_v (0 .. V).
 * A lane owns four consecutive columns of a row.  With W % 4 == 0 and maps and valid both 16-byte aligned every plane is stored as
 * 16-byte vectors, otherwise element by element; both paths store the same bits.  No atomics: the same bits on every run.
 * GE_ERR_BAD_ARG: null y_lr / pe / maps / valid; V outside {1, 2}; a size <= 0.  Checked before any launch.
 */
int ge_ground_maps(const float* logits_lr, const float* y_lr, const float* pe, long pe_bs, const float* height, float depth_scale,
                   float gain, int flip, float* maps, uint8_t* valid, int V, int h, int w, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_GROUND_H */
