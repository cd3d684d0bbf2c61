// Scene clouds (tools/misc/visualize_point-cloud_kitti_gt_pe_pred.py of the reference; include/gedepth_scene.h): the kept points of up to
// four depth layers over one candidate grid — the prediction coloured from the frame, the ground-plane prior, the LiDAR ground truth
// (uint16, divided here) and the slope-adjusted ground plane in constant colours — as ONE hole-free buffer of 16-byte PLY records, layer
// after layer, each layer in row-major candidate order.
//
// cloud.hip's ordered two-launch compaction with the layer on blockIdx.y.  The layers' pointers, windows, ranges and colours travel BY VALUE
// in the kernel-argument block (SceneLayers, 4 x 48 = 192 bytes; a workgroup reads its layer's entry at a uniform offset), as BatchTable
// does in infer_batch.hip: no device-side table, nothing to keep alive after the call.
//   pass 1  block (l, b): the kept candidates of span b of layer l -> ws[l * blocks + b];
//   pass 2  block (l, b) folds the entries before l * blocks + b, in two sums (the layers before its own, its own layer's earlier spans),
//           forms the predicate again and places a kept lane at  fold + kept in earlier rounds + kept in earlier waves of the round +
//           kept in lower lanes (mbcnt of the ballot), one 16-byte store per kept point; the last block of a layer stores the layer's
//           count, the last block of the last layer the total as well.
// No atomics, no block waiting on another block, no grid-striding (the span grows as in cloud_geometry), so a point's place is a pure
// function of (layer, candidate index).  The candidate grid, the keep rule and the record are cloud_points.h's: a point has the bits
// ge_depth_points gives it.  Streaming work (at 352 x 1216 with four layers: 6 MB read, up to 27 MB written): launch-latency-sized.
#pragma clang fp contract(off)
#include "cloud_points.h"
#include "../../include/gedepth_scene.h"

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

// pass 2: the records; counts[l] from the block that owns layer l's last candidate, counts[L] from the last layer's
__global__ void __launch_bounds__(256) scene_write_k(SceneLayers t, const uint8_t* __restrict__ bgr, SceneArgs a, const int* __restrict__ ws,
                                                     ge_u32x4* __restrict__ records, int* __restrict__ counts) {
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
    if (blockIdx.y == gridDim.y - 1) counts[gridDim.y] = run;
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

extern "C" int ge_scene_points(const GeSceneLayer* layers, int L, int H, int W, const uint8_t* bgr, int Hs, int Ws, int top, int left, float fx,
                               float fy, float cx, float cy, int row0, int step, int alpha, void* records, int* counts, void* workspace,
                               void* stream) {
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
  scene_write_k<<<grid, 256, 0, s>>>(t, bgr, a, (const int*)workspace, (ge_u32x4*)records, counts);
  GE_LAUNCH_CHECK();
  return GE_OK;
}
