// What the point-cloud kernels share (cloud.hip: one depth map; scene.hip: up to four layers in one buffer): the candidate grid, the keep
// rule, the record and the span geometry, so that a point gets the same bits from either.  The arithmetic is numpy's float32 arithmetic:
// true IEEE division, no contraction (the pragma below holds for the rest of the including file too).
#pragma once
#pragma clang fp contract(off)
#include "common.h"

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
static inline bool cloud_geometry(int H, int W, int row0, int step, int& nc, int& n, int& ipt, unsigned& blocks) {
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
