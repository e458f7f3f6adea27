// Device helpers of the byte-oriented codecs (png.hip, png_decode.hip, jpeg_enc.hip): the scans and sums of 256-thread
// workgroups, the kernel that turns file sizes into offsets, and the frame geometry the three share.  Not for common.h, which
// every MFMA kernel includes twice.  Everything here has internal linkage: include it inside no namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace {

constexpr int kMaxPixels = 1 << 26;     // per frame; the PNG encoder's 9 (W + 1) H bits then stay below 2^32

inline bool geometry_ok(int frames, int H, int W) { return frames >= 1 && H >= 1 && W >= 1 && (long)H * W <= kMaxPixels; }

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// inclusive prefix sum over the 64 lanes of a wave (T: unsigned or unsigned long long)
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Exclusive prefix sum of one value per thread over a 256-thread workgroup, on top of `carry` (the total of the steps before
// this one); `carry` then moves on by this step's total.  Every thread of the workgroup must call it.  s_wave: 4 words of LDS,
// free for the next call on return.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* s_wave, T& carry) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const T incl = wave_incl_scan(v);
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  T before = carry;
  for (int k = 0; k < wv; ++k) before += s_wave[k];
  carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  __syncthreads();
  return before + incl - v;
}

// workgroup-wide sum of one unsigned per thread (256 threads); every thread gets the total
__device__ __forceinline__ unsigned group_sum(unsigned v, unsigned* s_wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// one workgroup: exclusive scan of the files' sizes -> offsets[0..frames]
__global__ __launch_bounds__(256) void k_codec_offsets(const unsigned long long* __restrict__ sizes, int frames, long long* __restrict__ offsets) {
  __shared__ unsigned long long s_wave[4];
  unsigned long long carry = 0;
  for (int f0 = 0; f0 < frames; f0 += 256) {
    const int f = f0 + threadIdx.x;
    const unsigned long long at = block_excl_scan(f < frames ? sizes[f] : 0ull, s_wave, carry);
    if (f < frames) offsets[f] = (long long)at;
  }
  if (threadIdx.x == 0) offsets[frames] = (long long)carry;
}

}  // namespace
