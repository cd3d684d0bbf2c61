// The frame table of the kernels that take up to GE_BATCH_MAX = 8 frames per launch, the frame index on blockIdx.y (infer.hip: front end;
// eval.hip: metric sums).  The frames of a batch differ in size (the KITTI days are 375 x 1242, 370 x 1224, 374 x 1238, 376 x 1241), crop
// offsets and ground depth, so each has its own pointers and geometry.  They travel BY VALUE in the kernel-argument struct: BatchTable is
// 8 x 32 = 256 bytes of the kernarg segment, which the host fills from the caller's array at launch.  A workgroup reads its frame's entry
// with scalar loads at a uniform offset; there is no device-side pointer table to keep alive and no host-to-device copy ordered before
// the launch.  A single-frame entry point is the table of one frame.
#pragma once
#include "common.h"
#include "../../include/gedepth_batch.h"

struct BatchTable { GeBatchFrame f[GE_BATCH_MAX]; };
static_assert(sizeof(GeBatchFrame) == 32 && sizeof(BatchTable) == 256, "the by-value frame table is 8 x {two pointers, four ints}");

// 0, or the error of a frame list: null list / n outside 1 .. GE_BATCH_MAX / a null image / (need_aux) a null aux / a window outside its frame
static inline int batch_frames_check(const GeBatchFrame* frames, int n, int Hc, int Wc, bool need_aux) {
  if (!frames || n < 1 || n > GE_BATCH_MAX || Hc <= 0 || Wc <= 0) return GE_ERR_BAD_ARG;
  for (int f = 0; f < n; ++f) {
    const GeBatchFrame& fr = frames[f];
    if (!fr.image || (need_aux && !fr.aux) || fr.H <= 0 || fr.W <= 0 || fr.top < 0 || fr.left < 0) return GE_ERR_BAD_ARG;
    if (Hc > fr.H - fr.top || Wc > fr.W - fr.left) return GE_ERR_BAD_ARG;
  }
  return GE_OK;
}
static inline BatchTable batch_table(const GeBatchFrame* frames, int n) {
  BatchTable t;
  for (int f = 0; f < GE_BATCH_MAX; ++f) t.f[f] = frames[f < n ? f : 0];     // entries >= n are never read (grid.y = n)
  return t;
}
