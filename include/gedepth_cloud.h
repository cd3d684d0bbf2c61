/*
 * gedepth_cloud.h — C ABI of the point-cloud entry points of libgedepth_hip.so (csrc/scene.hip, where
 * ge_depth_points is the scene cloud of gedepth_scene.h with one f32 layer coloured from the frame).
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Like gedepth_eval.h and gedepth_ddad.h, this header stands
 * beside the versioned training / inference ABI of gedepth_hip.h: none of the three changes with these entry points.
 */
#ifndef GEDEPTH_CLOUD_H
#define GEDEPTH_CLOUD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ge_depth_points: back-project a depth map through the camera intrinsics into a hole-free array of 16-byte records, the payload of a
 * binary little-endian PLY file with the properties x y z (float) red green blue alpha (uchar).
 *
 *   candidates   map pixels (r, c), r = row0, row0 + step, ... < H and c = 0, step, ... < W, in row-major order;
 *   kept         a candidate with dmin <= z && z <= dmax, z = depth[r, c] (f32 comparisons: NaN fails, +-inf fail finite bounds);
 *   record k     (the k-th kept candidate in that order) at records + 16 k:
 *                  x = ((float)c - cx) / fx * z,  y = ((float)r - cy) / fy * z,  z      three little-endian f32, computed in f32 in exactly
 *                                                                                       that order, true division, no contraction;
 *                  R, G, B, alpha                 four bytes; R, G, B = bytes 2, 1, 0 of frame pixel (top + r, left + c), or 255 each when
 *                                                 bgr is NULL;
 *   depth        (H, W) f32, 4-byte aligned;       bgr  (Hs, Ws, 3) uint8 BGR frame or NULL;
 *   fx fy cx cy  intrinsics in MAP coordinates (the frame's cx - left, cy - top);
 *   records      16-byte aligned, room for every candidate: 16 * ceil((H - row0) / step) * ceil(W / step) bytes; bytes beyond
 *                16 * count are not written;
 *   count        one int, written on the device: the number of kept candidates;
 *   workspace    ge_depth_points_workspace(H, W, row0, step) bytes, 4-byte aligned; every word a call reads it has written before.
 * Two launches, no atomics, no waiting between blocks: the order and the bytes are the same on every run.
 * GE_ERR_BAD_ARG: null depth / records / count / workspace; a size <= 0; row0 outside [0, H); step < 1; alpha outside [0, 255]; fx == 0 or
 * fy == 0; dmin > dmax; with bgr: a negative offset, top + H > Hs or left + W > Ws.
 * GE_ERR_UNSUPPORTED: records not 16-byte aligned; depth not 4-byte aligned; H * W beyond int.
 */
int ge_depth_points(const float* depth, int H, int W, const uint8_t* bgr, int Hs, int Ws, int top, int left, float fx, float fy, float cx,
                    float cy, float dmin, float dmax, int row0, int step, int alpha, void* records, int* count, void* workspace,
                    void* stream);
size_t ge_depth_points_workspace(int H, int W, int row0, int step);   /* bytes of `workspace`; 0 for arguments ge_depth_points refuses */

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_CLOUD_H */
