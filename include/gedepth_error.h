/*
 * gedepth_error.h — C ABI of the error images and the split-level error planes of libgedepth_hip.so (csrc/error.hip): where in the picture
 * a KITTI prediction is wrong.  ge_error_image[_batch] paints every LiDAR return of one frame with the band of its abs-rel error on the
 * frame's own pixels; ge_error_accumulate[_batch] adds the abs-rel error of every return into a per-pixel sum and count over a split.
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by the
 * caller, `stream` a hipStream_t, nothing allocates or synchronises, every check comes before a launch).  Declared here and not in
 * gedepth_hip.h: that header is the versioned training / inference ABI, and it does not change with these.
 *
 * pred, gt_raw, the window at (top, left), the rectangle r0, r1, c0, c1 and depth_scale, min_depth, max_depth are ge_depth_metrics'
 * (gedepth_eval.h).  All arithmetic is f32 with `fp contract(off)`:
 *
 *   counted pixel  ge_depth_metrics' rule: inside the rectangle, gt = (float)raw / depth_scale, gt > min_depth && gt < max_depth.
 *   error          e = fabsf(gt - p) / gt, n = e / tau, both true IEEE divisions.  tau is a caller's parameter in (0, 1] (0.05 in the Python
 *                  layers: n == 1 is 5 % abs-rel).  n != n gives n = +inf: a NaN prediction is the worst error, not an invisible one.
 *   band           #{ j : n >= T[j] }, T = 0.0625, 0.125, 0.25, 0.5, 1, 2, 4, 8, 16: 0 .. 9, a value on a threshold in the upper band.
 *   colours        ColorBrewer RdYlBu-10 from blue (band 0) to red (band 9), as RGB (49,54,149) (69,117,180) (116,173,209) (171,217,233)
 *                  (224,243,248) (254,224,144) (253,174,97) (244,109,67) (215,48,39) (165,0,38); stored as BGR uint8.
 *   dilation       output pixel (r, c) of the crop shows N = max n over the counted pixels (r', c') of the crop with |r - r'| <= radius and
 *                  |c - c'| <= radius, radius 0 .. 3: the worst return wins, whatever the order.  A destination may lie outside the
 *                  rectangle, a source may not.
 *   background     a pixel with no counted pixel in its window shows the frame's pixel (top + r, left + c): 0 as it is, 1 every channel
 *                  >> 1, 2 black.
 *   err plane      (Hc, Wc) f32, optional: e at the counted pixels before dilation (a NaN stays NaN), -1.f elsewhere.
 *   accumulators   sum (Hc, Wc) f64, count (Hc, Wc) uint32.  For each image of the call in index order, at each counted pixel with a FINITE
 *                  e: sum += (double)e, count += 1.  A NaN or infinite e enters neither plane.  No atomics: a thread owns four pixels and
 *                  walks the call's images in order, so the planes equal a sequential float64 sum in frame order bit for bit, however the
 *                  frames were split into calls.
 */
#ifndef GEDEPTH_ERROR_H
#define GEDEPTH_ERROR_H

#include <stddef.h>
#include <stdint.h>

#include "gedepth_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GE_ERROR_BANDS 10
#define GE_ERROR_MAX_RADIUS 3

/*
 * ge_error_image: one image, one launch.
 *   image     the frame's (H, W, 3) uint8 BGR pixels; may be null only with background == 2;
 *   out       (Hc, Wc, 3) uint8 BGR, every byte written; stored four pixels as three 4-byte words where out is 4-byte aligned and
 *             Wc % 4 == 0, else byte by byte;
 *   err       (Hc, Wc) f32, every element written, or null.
 * GE_ERR_BAD_ARG: a null pred, gt_raw or out, a null image with background 0 or 1, a non-positive size, a window outside (H, W), a
 * rectangle outside the crop, radius outside 0 .. 3, background outside 0 .. 2, a tau that is NaN, <= 0 or > 1.  GE_ERR_UNSUPPORTED: pred
 * or err not 4-byte aligned, gt_raw not 2-byte aligned.
 */
int ge_error_image(const float* pred, const uint16_t* gt_raw, const uint8_t* image, int H, int W, int top, int left, int Hc, int Wc,
                   int r0, int r1, int c0, int c1, float depth_scale, float min_depth, float max_depth, float tau, int radius, int background,
                   uint8_t* out, float* err, void* stream);

/*
 * ge_error_image_batch: the same kernel for n images in the same single launch (the image on blockIdx.y), as ge_depth_metrics_batch is to
 * ge_depth_metrics: block f of out (n, Hc, Wc, 3) and err (n, Hc, Wc) carries the bytes ge_error_image gives image f.  pred (n, Hc, Wc)
 * f32; frames[f].image the (H, W) uint16 ground truth of image f, frames[f].aux its (H, W, 3) uint8 BGR frame: none null, or any of
 * them null with background == 2.
 * GE_ERR_BAD_ARG as above, and n outside 1 .. GE_BATCH_MAX.  GE_ERR_UNSUPPORTED as above, and Wc % 4 != 0 or pred not 16-byte aligned.
 */
int ge_error_image_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                         float depth_scale, float min_depth, float max_depth, float tau, int radius, int background, uint8_t* out, float* err,
                         void* stream);

/*
 * ge_error_accumulate: one image into the planes, one launch.  sum (Hc, Wc) f64, 8-byte aligned; count (Hc, Wc) uint32, 4-byte aligned;
 * both updated in place with plain loads and stores (the caller zeroes them before a split).  A pixel that no image of the call counts
 * with a finite e is not stored to.
 * GE_ERR_BAD_ARG: a null pointer, a non-positive size, a window outside (H, W), a rectangle outside the crop.  GE_ERR_UNSUPPORTED: pred not
 * 4-byte aligned, gt_raw not 2-byte aligned, sum not 8-byte or count not 4-byte aligned.
 */
int ge_error_accumulate(const float* pred, const uint16_t* gt_raw, int H, int W, int top, int left, int Hc, int Wc, int r0, int r1, int c0,
                        int c1, float depth_scale, float min_depth, float max_depth, double* sum, uint32_t* count, void* stream);

/*
 * ge_error_accumulate_batch: n images (frames[f].image the ground truth; aux is not read) into the same planes in one launch, image 0
 * first.  The planes afterwards hold the bits of n ge_error_accumulate calls in index order.
 * GE_ERR_BAD_ARG as above, and n outside 1 .. GE_BATCH_MAX.  GE_ERR_UNSUPPORTED as above, and Wc % 4 != 0 or pred not 16-byte aligned.
 */
int ge_error_accumulate_batch(const float* pred, const GeBatchFrame* frames, int n, int Hc, int Wc, int r0, int r1, int c0, int c1,
                              float depth_scale, float min_depth, float max_depth, double* sum, uint32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_ERROR_H */
