// What the kernels on uint8 label stacks share (label_census.hip, label_pairs.hip, label_components.hip, and through
// label_scan.h label_polygons.hip and rle.hip): the workgroup, the limits of a stack, and for those that walk it 16 bytes per
// lane the byte compares of a lane's piece, the wave's integer sum, minimum and maximum, the unaligned word and the bound on the grid.
#pragma once
#include "common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxFrames = 65535;
constexpr long kMaxPixels = 1L << 26;
constexpr int kMaxBlocks = 2048;      // workgroups of one launch, about: enough to fill the chip, few enough to keep the flushes rare

// host: a stack of n frames of H x W that the entry points take
inline bool stack_geometry_ok(int n, int H, int W) { return n >= 1 && n <= kMaxFrames && H >= 1 && W >= 1 && (long)H * W <= kMaxPixels; }

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// four bytes that may start anywhere, as one little-endian word
__device__ __forceinline__ uint32_t load4(const unsigned char* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// bit j = byte j of w equals the byte replicated in v4
__device__ __forceinline__ unsigned eq4(uint32_t w, uint32_t v4) {
  const uint32_t t = w ^ v4;
  const uint32_t z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu);   // 0x80 in every zero byte of t, exactly
  return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;
}
// bit j = byte j (0..15) of w equals v
__device__ __forceinline__ unsigned eq16(uint4 w, int v) {
  const uint32_t v4 = (uint32_t)v * 0x01010101u;
  return eq4(w.x, v4) | (eq4(w.y, v4) << 4) | (eq4(w.z, v4) << 8) | (eq4(w.w, v4) << 12);
}
__device__ __forceinline__ bool all_equal(uint4 w) {
  return w.x == w.y && w.x == w.z && w.x == w.w && w.x == ((w.x >> 8) | (w.x << 24));
}
// byte j (0..15) of w, without indexing registers dynamically
__device__ __forceinline__ int byte_at(uint4 w, int j) {
  const uint32_t word = j < 8 ? (j < 4 ? w.x : w.y) : (j < 12 ? w.z : w.w);
  return (int)((word >> (8 * (j & 3))) & 0xffu);
}

// workgroups per frame: one 16-byte piece per thread at the finest, about kMaxBlocks in the whole launch at the coarsest
inline int blocks_per_frame(long pixels, int n) {
  const long chunks = pixels / 16 + 1;
  long b = (chunks + kThreads - 1) / kThreads;
  const long cap = kMaxBlocks / n > 1 ? kMaxBlocks / n : 1;
  if (b > cap) b = cap;
  return (int)b;
}
}  // namespace
