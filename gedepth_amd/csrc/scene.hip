// Point clouds from depth maps (tools/misc/visualize_point-cloud_kitti.py and visualize_point-cloud_kitti_gt_pe_pred.py of the reference;
// include/gedepth_cloud.h, include/gedepth_scene.h; gedepth_amd/depth/utils/point_cloud.py here): back-project the pixels whose depth is in
// range through the intrinsics and leave them as 16-byte records (x y z f32, R G B alpha u8) with no holes: the device buffer is the
// payload of a binary PLY file byte for byte.  A scene is the kept points of up to four depth layers over one candidate grid — the
// prediction coloured from the frame, the ground-plane prior, the LiDAR ground truth (uint16, divided here) and the slope-adjusted ground
// plane in constant colours — layer after layer, each layer in row-major candidate order.  ge_depth_points is the scene of one f32 layer
// coloured from the frame.
//
// Ordered stream compaction in two launches with the layer on blockIdx.y.  A block owns a contiguous span of 256 * ipt candidates of its
// layer, taken 256 at a time (thread t of round j: candidate span start + 256 j + t, so a wave reads 64 neighbours).  The layers' pointers,
// windows, ranges and colours travel BY VALUE in the kernel-argument block (SceneLayers, 4 x 48 = 192 bytes; a workgroup reads its layer's
// entry at a uniform offset), as BatchTable does in batch_table.h: no device-side table, nothing to keep alive after the call.
//   pass 1  block (l, b): predicate -> 64-bit ballot -> popcount per wave, the four wave counts through LDS, the kept candidates of span b
//           of layer l -> ws[l * blocks + b];
//   pass 2  block (l, b) folds the entries before l * blocks + b, in two sums (the layers before its own, its own layer's earlier spans),
//           forms the predicate again and places a kept lane at  fold + kept in earlier rounds + kept in earlier waves of the round +
//           kept in lower lanes (mbcnt of the ballot), one 16-byte store per kept point; the last block of a layer stores the layer's
//           count, the last block of the last layer the total as well, where the caller has room for one.
// No atomics, no block waiting on another block; the grid is capped by growing ipt, never by grid-striding, so a point's place is a pure
// function of (layer, candidate index).  The arithmetic is numpy's float32 arithmetic: true IEEE division, no contraction.  Streaming work
// (at 352 x 1216 with four layers: 6 MB read, up to 27 MB written): launch-latency-sized.
#pragma clang fp contract(off)
#include "common.h"
#include "../../include/gedepth_cloud.h"
#include "../../include/gedepth_scene.h"

#define GE_CLOUD_MIN_IPT 4          // candidates per thread: at least 4 (a span of 1024), more once the grid would pass GE_CLOUD_MAX_BLOCKS
#define GE_CLOUD_MAX_BLOCKS 1024

// candidate i (< the number of candidates) of the grid r = row0, row0 + step, ..., c = 0, step, ... with nc candidates per row -> its pixel
__device__ __forceinline__ void cloud_pixel(int i, int nc, int row0, int step, int& r, int& c) {
  const int ri = i / nc;
  r = row0 + ri * step;
  c = (i - ri * nc) * step;
}

// the keep rule: f32 comparisons, so NaN fails and +-inf fail finite bounds
__device__ __forceinline__ bool cloud_in_range(float z, float dmin, float dmax) { return dmin <= z && z <= dmax; }

// R | G << 8 | B << 16 of the BGR frame's pixel (top + r, left + c); white without a frame
__device__ __forceinline__ uint32_t cloud_frame_rgb(const uint8_t* __restrict__ bgr, int Ws, int top, int left, int r, int c) {
  if (!bgr) return 0x00ffffffu;
  const uint8_t* p = bgr + ((long)(top + r) * Ws + (left + c)) * 3;
  return (uint32_t)p[2] | ((uint32_t)p[1] << 8) | ((uint32_t)p[0] << 16);
}

// the 16-byte record of pixel (r, c) at depth z: x y z f32, then R G B alpha
__device__ __forceinline__ ge_u32x4 cloud_record(int r, int c, float z, float fx, float fy, float cx, float cy, uint32_t rgb, uint32_t alpha) {
  const float x = ((float)c - cx) / fx * z;
  const float y = ((float)r - cy) / fy * z;
  const ge_u32x4 rec = {__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), rgb | (alpha << 24)};
  return rec;
}

// the number of set bits of a wave's ballot below this lane
__device__ __forceinline__ int cloud_lower_lanes(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// nc, n, ipt and the blocks per map of a geometry; false for one the entry points refuse.  The grid is capped by growing ipt, never by
// grid-striding, so a point's place is a pure function of its candidate index.
static bool cloud_geometry(int H, int W, int row0, int step, int& nc, int& n, int& ipt, unsigned& blocks) {
  if (H <= 0 || W <= 0 || row0 < 0 || row0 >= H || step < 1 || (long)H * W > 0x7fffffffL) return false;
  const long nr = ((long)(H - row0) + step - 1) / step;
  nc = (int)(((long)W + step - 1) / step);
  n = (int)(nr * nc);                                 // <= H * W
  const long per = 256L * GE_CLOUD_MAX_BLOCKS;
  ipt = (int)((n + per - 1) / per);
  if (ipt < GE_CLOUD_MIN_IPT) ipt = GE_CLOUD_MIN_IPT;
  blocks = (unsigned)((n + 256L * ipt - 1) / (256L * ipt));
  return true;
}

struct SceneLayers { GeSceneLayer l[GE_SCENE_MAX_LAYERS]; };
static_assert(sizeof(GeSceneLayer) == 48 && sizeof(SceneLayers) == 192, "the by-value layer table is 4 x 48 bytes");

extern "C" size_t ge_scene_layer_size(void) { return sizeof(GeSceneLayer); }

struct SceneArgs {
  int nc, n, row0, step, ipt;       // nc candidates per row, n per layer
  int Ws, top, left;                // the frame
  float fx, fy, cx, cy;
  uint32_t alpha;
};

// candidate i of layer ly -> its pixel, its depth and whether it is kept (false beyond the last candidate)
__device__ __forceinline__ bool scene_keep(const GeSceneLayer& ly, const SceneArgs& a, long i, int& r, int& c, float& z) {
  if (i >= a.n) return false;
  cloud_pixel((int)i, a.nc, a.row0, a.step, r, c);
  const long e = (long)(ly.top + r) * ly.W + (ly.left + c);
  z = ly.kind == GE_SCENE_U16 ? (float)((const uint16_t*)ly.data)[e] / ly.scale : ((const float*)ly.data)[e];
  return cloud_in_range(z, ly.dmin, ly.dmax);
}

// pass 1: ws[l * blocks + b] = the number of kept candidates of span b of layer l
__global__ void __launch_bounds__(256) scene_count_k(SceneLayers t, SceneArgs a, int* __restrict__ ws) {
  __shared__ int wc[4];
  const GeSceneLayer ly = t.l[blockIdx.y];
  const long base = (long)blockIdx.x * a.ipt * 256 + threadIdx.x;
  int cnt = 0;                                        // the same in every lane of a wave
  for (int j = 0; j < a.ipt; ++j) {
    int r, c;
    float z;
    cnt += __popcll(__ballot(scene_keep(ly, a, base + 256 * j, r, c, z)));
  }
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.y * gridDim.x + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// pass 2: the records; counts[l] from the block that owns layer l's last candidate, *total (unless null) from the last layer's
__global__ void __launch_bounds__(256) scene_write_k(SceneLayers t, const uint8_t* __restrict__ bgr, SceneArgs a, const int* __restrict__ ws,
                                                     ge_u32x4* __restrict__ records, int* __restrict__ counts, int* __restrict__ total) {
  __shared__ int red[2][256];                         // [0]: the layers before this one, [1]: this layer's earlier spans
  __shared__ int wc[2][4];                            // the wave counts of a round; two sets, so one barrier per round is enough
  const int t_ = threadIdx.x, lane = t_ & 63, w = t_ >> 6;
  const GeSceneLayer ly = t.l[blockIdx.y];
  const int first = (int)(blockIdx.y * gridDim.x), own = first + (int)blockIdx.x;     // <= 4 * 1024 entries
  int s0 = 0, s1 = 0;
  for (int p = t_; p < own; p += 256) {
    const int v = ws[p];
    if (p < first) s0 += v; else s1 += v;
  }
  red[0][t_] = s0;
  red[1][t_] = s1;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t_ < h) { red[0][t_] += red[0][t_ + h]; red[1][t_] += red[1][t_ + h]; }
    __syncthreads();
  }
  const int before = red[0][0];                       // kept points of the layers before this one
  int run = before + red[1][0];                       // kept points before this round
  const uint8_t* frame = ly.from_frame ? bgr : nullptr;
  const uint32_t rgb = (uint32_t)ly.red | ((uint32_t)ly.green << 8) | ((uint32_t)ly.blue << 16);
  const long base = (long)blockIdx.x * a.ipt * 256 + t_;
  for (int j = 0; j < a.ipt; ++j) {
    int r = 0, c = 0;
    float z = 0.f;
    const bool keep = scene_keep(ly, a, base + 256 * j, r, c, z);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[j & 1][w] = __popcll(m);
    __syncthreads();
    const int c0 = wc[j & 1][0], c1 = wc[j & 1][1], c2 = wc[j & 1][2], c3 = wc[j & 1][3];
    if (keep) {
      const long k = (long)run + (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + cloud_lower_lanes(m);
      const uint32_t colour = ly.from_frame ? cloud_frame_rgb(frame, a.Ws, a.top, a.left, r, c) : rgb;
      records[k] = cloud_record(r, c, z, a.fx, a.fy, a.cx, a.cy, colour, a.alpha);
    }
    run += c0 + c1 + c2 + c3;
  }
  if (blockIdx.x == gridDim.x - 1 && t_ == 0) {
    counts[blockIdx.y] = run - before;
    if (blockIdx.y == gridDim.y - 1 && total) *total = run;
  }
}

// cloud_geometry for L layers; false for what ge_scene_points refuses on the grid's account (L * n beyond int: the total is an int)
static bool scene_geometry(int H, int W, int row0, int step, int L, int& nc, int& n, int& ipt, unsigned& blocks) {
  if (L < 1 || L > GE_SCENE_MAX_LAYERS || !cloud_geometry(H, W, row0, step, nc, n, ipt, blocks)) return false;
  return (long)L * n <= 0x7fffffffL;
}

extern "C" size_t ge_scene_points_workspace(int H, int W, int row0, int step, int L) {
  int nc, n, ipt;
  unsigned blocks;
  if (!scene_geometry(H, W, row0, step, L, nc, n, ipt, blocks)) return 0;
  return (size_t)L * blocks * sizeof(int);
}

// ge_scene_points but for the total: counts[L] with `with_total`, nowhere without (ge_depth_points: `counts` is one int)
static int scene_points(const GeSceneLayer* layers, int L, int H, int W, const uint8_t* bgr, int Hs, int Ws, int top, int left, float fx, float fy,
                        float cx, float cy, int row0, int step, int alpha, void* records, int* counts, bool with_total, void* workspace, void* stream) {
  if (!layers || !records || !counts || !workspace || L < 1 || L > GE_SCENE_MAX_LAYERS || H <= 0 || W <= 0 || row0 < 0 || row0 >= H ||
      step < 1 || alpha < 0 || alpha > 255 || fx == 0.f || fy == 0.f)
    return GE_ERR_BAD_ARG;
  if (bgr && (Hs <= 0 || Ws <= 0 || top < 0 || left < 0 || top > Hs - H || left > Ws - W)) return GE_ERR_BAD_ARG;   // no overflow: Hs - H
  for (int l = 0; l < L; ++l) {
    const GeSceneLayer& ly = layers[l];
    if (!ly.data || (ly.kind != GE_SCENE_F32 && ly.kind != GE_SCENE_U16) || ly.H <= 0 || ly.W <= 0 || ly.top < 0 || ly.left < 0 ||
        ly.top > ly.H - H || ly.left > ly.W - W || ly.dmin > ly.dmax || (ly.kind == GE_SCENE_U16 && ly.scale == 0.f))
      return GE_ERR_BAD_ARG;
  }
  for (int l = 0; l < L; ++l)
    if ((uintptr_t)layers[l].data & (layers[l].kind == GE_SCENE_U16 ? 1 : 3)) return GE_ERR_UNSUPPORTED;
  SceneArgs a;
  unsigned blocks;
  if (((uintptr_t)records & 15) || !scene_geometry(H, W, row0, step, L, a.nc, a.n, a.ipt, blocks)) return GE_ERR_UNSUPPORTED;
  a.row0 = row0; a.step = step;
  a.Ws = Ws; a.top = top; a.left = left;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.alpha = (uint32_t)alpha;
  SceneLayers t;
  for (int l = 0; l < GE_SCENE_MAX_LAYERS; ++l) t.l[l] = layers[l < L ? l : 0];     // entries >= L are never read (grid.y = L)
  hipStream_t s = ge_stream(stream);
  const dim3 grid(blocks, (unsigned)L);
  scene_count_k<<<grid, 256, 0, s>>>(t, a, (int*)workspace);
  GE_LAUNCH_CHECK();
  scene_write_k<<<grid, 256, 0, s>>>(t, bgr, a, (const int*)workspace, (ge_u32x4*)records, counts, with_total ? counts + L : nullptr);
  GE_LAUNCH_CHECK();
  return GE_OK;
}

extern "C" int ge_scene_points(const GeSceneLayer* layers, int L, int H, int W, const uint8_t* bgr, int Hs, int Ws, int top, int left, float fx,
                               float fy, float cx, float cy, int row0, int step, int alpha, void* records, int* counts, void* workspace,
                               void* stream) {
  return scene_points(layers, L, H, W, bgr, Hs, Ws, top, left, fx, fy, cx, cy, row0, step, alpha, records, counts, true, workspace, stream);
}

// the scene of one f32 layer: the whole map, coloured from the frame
extern "C" size_t ge_depth_points_workspace(int H, int W, int row0, int step) { return ge_scene_points_workspace(H, W, row0, step, 1); }

extern "C" int ge_depth_points(const float* depth, int H, int W, const uint8_t* bgr, int Hs, int Ws, int top, int left, float fx, float fy,
                               float cx, float cy, float dmin, float dmax, int row0, int step, int alpha, void* records, int* count,
                               void* workspace, void* stream) {
  GeSceneLayer ly = {};
  ly.data = depth; ly.kind = GE_SCENE_F32; ly.H = H; ly.W = W; ly.scale = 1.f; ly.dmin = dmin; ly.dmax = dmax; ly.from_frame = 1;
  return scene_points(&ly, 1, H, W, bgr, Hs, Ws, top, left, fx, fy, cx, cy, row0, step, alpha, records, count, false, workspace, stream);
}
