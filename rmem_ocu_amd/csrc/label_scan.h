// The workgroup scan of the kernels that count in one walk over a label stack and write in a second (rle.hip, label_polygons.hip),
// and the kernel both launch in between: the exclusive scan of a row of unit counters.  Not for label_wave.h: a __global__ in a
// header is emitted into every translation unit that includes it.  Everything here has internal linkage: include it inside no
// namespace.
#pragma once
#include "label_wave.h"

namespace {
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
// inclusive scan over the workgroup's kThreads values (thread order) and their total; sh: kWaves entries; whole workgroups only
template <typename T>
__device__ __forceinline__ T block_incl_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T w = wave_incl_scan(v, lane);
  __syncthreads();                    // the previous call's readers are done with sh
  if (lane == 63) sh[wave] = w;
  __syncthreads();
  T add = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const T s = sh[k];
    if (k < wave) add += s;
    tot += s;
  }
  total = tot;
  return w + add;
}

// one workgroup per row of U counters (cnt + blockIdx.x * U): exclusive scan in place, the row's total to totals[blockIdx.x]
__global__ __launch_bounds__(kThreads) void k_label_scan_units(int* __restrict__ cnt, int U, int* __restrict__ totals) {
  __shared__ int sh[kWaves];
  int* c = cnt + (size_t)blockIdx.x * U;
  int carry = 0;
  for (int b = 0; b < U; b += kThreads) {
    const int i = b + threadIdx.x;
    const int v = i < U ? c[i] : 0;
    int tot;
    const int inc = block_incl_scan(v, sh, tot);
    if (i < U) c[i] = carry + inc - v;
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}
}  // namespace
