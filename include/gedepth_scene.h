/*
 * gedepth_scene.h — C ABI of the scene-cloud entry points of libgedepth_hip.so (csrc/scene.hip): the points of up to four depth layers
 * over one candidate grid (the prediction, the ground-plane prior, the LiDAR ground truth, the slope-adjusted ground plane: role of the
 * reference's tools/misc/visualize_point-cloud_kitti_gt_pe_pred.py) in ONE hole-free record buffer, the payload of a binary PLY file.
 *
 * Same conventions as gedepth_hip.h (extern "C", 0 on success, GE_ERR_* of that header for argument errors, device pointers owned by
 * the caller, `stream` a hipStream_t, nothing allocates or synchronises).  Like gedepth_cloud.h, whose record and keep rule this header
 * shares (one kernel pair runs both), it stands beside the versioned training / inference ABI of gedepth_hip.h, which does not change with it.
 */
#ifndef GEDEPTH_SCENE_H
#define GEDEPTH_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GE_SCENE_MAX_LAYERS 4
#define GE_SCENE_F32 0   /* GeSceneLayer.kind: data is an (H, W) f32 array, 4-byte aligned */
#define GE_SCENE_U16 1   /*                    data is an (H, W) uint16 array, 2-byte aligned: z = (float)raw / scale, a true f32 division */

/*
 * One layer.  Candidate (r, c) of the grid reads element (top + r, left + c) of the layer's own (H, W) array; it is kept iff
 * dmin <= z && z <= dmax (f32 comparisons: NaN fails).  `scale` is ignored for an f32 layer.  Colour: from_frame != 0 takes R, G, B from the
 * frame as ge_depth_points does (white when bgr is NULL); from_frame == 0 gives every point of the layer the constant red, green, blue.
 * 48 bytes, no implicit padding.
 */
typedef struct GeSceneLayer {
  const void* data;
  int kind;
  int H, W, top, left;
  float scale, dmin, dmax;
  int from_frame;
  uint8_t red, green, blue, reserved;
} GeSceneLayer;

size_t ge_scene_layer_size(void);   /* sizeof(GeSceneLayer), for a binding to check its mirror of the struct against */

/*
 * ge_scene_points: the kept points of L layers, 1 <= L <= GE_SCENE_MAX_LAYERS, over one candidate grid.
 *
 *   candidates   map pixels (r, c), r = row0, row0 + step, ... < H and c = 0, step, ... < W, in row-major order, as in ge_depth_points;
 *   record       16 bytes, exactly ge_depth_points' (gedepth_cloud.h): x = ((float)c - cx) / fx * z, y = ((float)r - cy) / fy * z, z in
 *                f32, true division, no contraction; then R, G, B, alpha.  A single f32 layer with from_frame != 0 and a zero window
 *                gives ge_depth_points' bytes;
 *   layers       a HOST array of L layers, read during the call: they travel by value in the kernel-argument block (4 x 48 = 192 bytes),
 *                there is no device-side table, and the array may be reused as soon as the call returns;
 *   bgr          (Hs, Ws, 3) uint8 BGR frame or NULL; frame pixel (top + r, left + c) colours candidate (r, c) of a from_frame layer;
 *   fx fy cx cy  intrinsics in MAP coordinates;
 *   records      16-byte aligned, room for every candidate of every layer: 16 * L * ceil((H - row0) / step) * ceil(W / step) bytes.  All
 *                kept points of layer 0 come first, in candidate order, then all of layer 1, and so on, with no holes; bytes beyond
 *                16 * counts[L] are not written;
 *   counts       L + 1 ints, written on the device: the layers' kept counts, then their total;
 *   workspace    ge_scene_points_workspace(H, W, row0, step, L) bytes, 4-byte aligned; every word a call reads it has written before.
 * Two launches with the layer on blockIdx.y (one count per (layer, block); every block folds the counts before its own in layer-major
 * order and places its kept lanes by ballot), no atomics, no waiting between blocks: a point's place is a pure function of (layer,
 * candidate index), and the bytes are the same on every run.
 * GE_ERR_BAD_ARG: null layers / records / counts / workspace or a null layer's data; L outside 1 .. GE_SCENE_MAX_LAYERS; a size <= 0 (the
 * map's or a layer's); row0 outside [0, H); step < 1; alpha outside [0, 255]; fx == 0 or fy == 0; a layer with dmin > dmax, an unknown kind,
 * scale == 0 on a uint16 layer, or a window that leaves its array (a negative offset, top + H > the layer's H, left + W > its W); with bgr:
 * a frame window that leaves the frame.
 * GE_ERR_UNSUPPORTED: records not 16-byte aligned; f32 data not 4-byte aligned; uint16 data not 2-byte aligned; H * W beyond int, or L
 * times the number of candidates beyond int (the total is an int).
 * Every check comes before the first launch.
 */
int ge_scene_points(const GeSceneLayer* layers, int L, int H, int W, const uint8_t* bgr, int Hs, int Ws, int top, int left, float fx,
                    float fy, float cx, float cy, int row0, int step, int alpha, void* records, int* counts, void* workspace, void* stream);
size_t ge_scene_points_workspace(int H, int W, int row0, int step, int L);   /* bytes of `workspace`; 0 for arguments ge_scene_points refuses */

#ifdef __cplusplus
}
#endif
#endif /* GEDEPTH_SCENE_H */
