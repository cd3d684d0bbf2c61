// Gradient accumulation over several iterations (include/gedepth_accum.h): acc = grad or acc += grad over the optimizer's arena, with the
// squared norm of the result from the same pass when the window ends.  Pure HBM streaming: 8 B (first) or 12 B (add) per element.
#include "common.h"
#include "../../include/gedepth_accum.h"

#define ACC_THREADS 256
#define ACC_UNROLL 4                                      // float4 per thread and trip: 8 independent 16-byte loads in flight
#define ACC_PER_BLOCK (ACC_THREADS * ACC_UNROLL * 4)      // 4096 elements per workgroup and trip
#define ACC_MAX_BLOCKS 2048                               // one trip of the capped grid covers 2048 * 4096 = 8 388 608 elements

// FIRST and NORM are launch-uniform: the copy never loads acc, and without a norm there is no conversion, LDS or atomic in the kernel
template <bool FIRST, bool NORM>
__global__ void __launch_bounds__(ACC_THREADS) grad_accum_k(float* __restrict__ acc, const float* __restrict__ grad, long n,
                                                            double* __restrict__ sumsq) {
#pragma clang fp contract(off)
  const long n4 = n >> 2;
  float4* a4 = (float4*)acc;
  const float4* g4 = (const float4*)grad;
  double s = 0;
  // a workgroup takes whole tiles of ACC_UNROLL * ACC_THREADS consecutive float4 (16 KiB per array), a grid apart: what is in flight at any
  // time are contiguous runs, not ACC_UNROLL streams a power of two apart (8 MiB at the capped grid), which land on the same HBM channels
  for (long base = (long)blockIdx.x * (ACC_UNROLL * ACC_THREADS); base < n4; base += (long)gridDim.x * (ACC_UNROLL * ACC_THREADS)) {
    const long i = base + threadIdx.x;
    if (base + ACC_UNROLL * ACC_THREADS <= n4) {             // a full tile (workgroup-uniform): all loads issued before the first use
      float4 v[ACC_UNROLL], a[ACC_UNROLL];
#pragma unroll
      for (int u = 0; u < ACC_UNROLL; ++u) v[u] = g4[i + u * ACC_THREADS];
      if (!FIRST) {
#pragma unroll
        for (int u = 0; u < ACC_UNROLL; ++u) a[u] = a4[i + u * ACC_THREADS];
#pragma unroll
        for (int u = 0; u < ACC_UNROLL; ++u) { v[u].x = a[u].x + v[u].x; v[u].y = a[u].y + v[u].y; v[u].z = a[u].z + v[u].z; v[u].w = a[u].w + v[u].w; }
      }
#pragma unroll
      for (int u = 0; u < ACC_UNROLL; ++u) {
        a4[i + u * ACC_THREADS] = v[u];
        if (NORM) s += (double)v[u].x * v[u].x + (double)v[u].y * v[u].y + (double)v[u].z * v[u].z + (double)v[u].w * v[u].w;
      }
    } else {                                                 // the last, partial tile of the arena
      for (long j = i; j < n4; j += ACC_THREADS) {
        float4 v = g4[j];
        if (!FIRST) { const float4 a = a4[j]; v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w; }
        a4[j] = v;
        if (NORM) s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {          // the scalar tail
    const long t = (n4 << 2) + threadIdx.x;
    float v = grad[t];
    if (!FIRST) v = acc[t] + v;
    acc[t] = v;
    if (NORM) s += (double)v * v;
  }
  if (NORM) {
    __shared__ double sm[ACC_THREADS / GE_WAVE];
    s = ge_wave_sum(s);
    if ((threadIdx.x & (GE_WAVE - 1)) == 0) sm[threadIdx.x / GE_WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sumsq, sm[0] + sm[1] + sm[2] + sm[3]);
  }
}

extern "C" int ge_grad_accum(float* acc, const float* grad, long n, int first, double* sumsq, void* stream) {
  if (!acc || !grad || n < 0 || acc == grad || (((uintptr_t)acc | (uintptr_t)grad) & 15) || ((uintptr_t)sumsq & 7)) return GE_ERR_BAD_ARG;
  if (n == 0) return GE_OK;
  const unsigned blocks = ge_blocks(n, ACC_PER_BLOCK, ACC_MAX_BLOCKS);
  hipStream_t s = ge_stream(stream);
  if (first) {
    if (sumsq) grad_accum_k<true, true><<<blocks, ACC_THREADS, 0, s>>>(acc, grad, n, sumsq);
    else grad_accum_k<true, false><<<blocks, ACC_THREADS, 0, s>>>(acc, grad, n, nullptr);
  } else {
    if (sumsq) grad_accum_k<false, true><<<blocks, ACC_THREADS, 0, s>>>(acc, grad, n, sumsq);
    else grad_accum_k<false, false><<<blocks, ACC_THREADS, 0, s>>>(acc, grad, n, nullptr);
  }
  GE_LAUNCH_CHECK();
  return GE_OK;
}
