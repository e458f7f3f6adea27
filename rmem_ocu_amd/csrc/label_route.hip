// Label routing of a ragged clip group (include/rmem.h, rmem_route_labels): one launch moves every row's uint8 label map of a step
// where its clip keeps it, lays a new object's map over it, swaps in fed labels and mirrors the result into the row's flip twin.
// Element-type agnostic (uint8 in, uint8 out): built once.
#include "common.h"
#include "../../include/rmem.h"

namespace {
constexpr int kRouteThreads = 256;
constexpr long kRouteMaxPixels = 1L << 26;

__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// One thread = the 4 bytes [4k, 4k + 4) of a row's flat Ho * Wo map (the last group of a row may be shorter).  A row's operands
// (the row itself, feed, overlay, dst) are read / written as one 32-bit word per thread when ALL of them start 4-byte aligned --
// uniform per row, so a wave never diverges on it -- and byte by byte otherwise.  The mirrored group lands in the twin's row at
// other addresses (W - 1 - x): its own 32-bit store is taken when the four pixels lie in one image line and the reversed group
// starts aligned, single bytes otherwise.
__global__ __launch_bounds__(kRouteThreads) void k_route_labels(unsigned char* rows_u8, int rows, int n, int Wo,
                                                                const rmem_label_route* __restrict__ routes) {
  const int r = blockIdx.y;
  const rmem_label_route rt = routes[r];
  if (rt.mode != 0 && rt.mode != 1) return;
  unsigned char* row = rows_u8 + (size_t)r * n;
  const int p = 4 * (blockIdx.x * kRouteThreads + threadIdx.x);
  if (p >= n) return;
  const int m = n - p < 4 ? n - p : 4;
  if (rt.mode == 1) {
    if (m == 4 && aligned4(row)) *(uint32_t*)(row + p) = 0u;
    else for (int j = 0; j < m; ++j) row[p + j] = 0;
    return;
  }
  const unsigned char* feed = rt.feed;
  const unsigned char* over = rt.overlay;
  unsigned char* dst = rt.dst;
  const bool wide = m == 4 && aligned4(row) && (!feed || aligned4(feed)) && (!over || aligned4(over)) && (!dst || aligned4(dst));
  uint32_t pred = 0, fd = 0, ov = 0;
  if (wide) {
    pred = *(const uint32_t*)(row + p);
    if (feed) fd = *(const uint32_t*)(feed + p);
    if (over) ov = *(const uint32_t*)(over + p);
  } else {
    for (int j = 0; j < m; ++j) {
      pred |= (uint32_t)row[p + j] << (8 * j);
      if (feed) fd |= (uint32_t)feed[p + j] << (8 * j);
      if (over) ov |= (uint32_t)over[p + j] << (8 * j);
    }
  }
  uint32_t x = feed ? fd : pred;
  if (over) {
    uint32_t keep = 0;                 // 0xff in every byte where the overlay is zero
#pragma unroll
    for (int j = 0; j < 4; ++j) keep |= ((ov >> (8 * j)) & 0xffu) ? 0u : 0xffu << (8 * j);
    x = (x & keep) | (ov & ~keep);
  }
  const uint32_t out = feed ? pred : x;
  if (wide) {
    *(uint32_t*)(row + p) = x;
    if (dst) *(uint32_t*)(dst + p) = out;
  } else {
    for (int j = 0; j < m; ++j) {
      row[p + j] = (unsigned char)(x >> (8 * j));
      if (dst) dst[p + j] = (unsigned char)(out >> (8 * j));
    }
  }
  const int twin = rt.twin;
  if (twin < 0 || twin >= rows || twin == r) return;
  unsigned char* trow = rows_u8 + (size_t)twin * n;
  const int y = p / Wo, x0 = p - y * Wo;
  if (m == 4 && x0 + 3 < Wo) {         // one image line: pixels x0 .. x0 + 3 go to W - 1 - x0 .. W - 4 - x0, reversed
    unsigned char* t = trow + (size_t)y * Wo + (Wo - 4 - x0);
    if (aligned4(t)) {
      *(uint32_t*)t = __builtin_bswap32(x);
      return;
    }
  }
  for (int j = 0; j < m; ++j) {
    const int q = p + j, yy = q / Wo, xx = q - yy * Wo;
    trow[(size_t)yy * Wo + (Wo - 1 - xx)] = (unsigned char)(x >> (8 * j));
  }
}
}  // namespace

extern "C" int rmem_route_labels(unsigned char* rows_u8, int rows, int Ho, int Wo, const rmem_label_route* routes, void* stream) {
  RMEM_REQUIRE(rows >= 1 && rows <= 65535, "rmem_route_labels: rows must be in 1..65535");
  RMEM_REQUIRE(rows_u8 && routes, "rmem_route_labels: null pointer (rows_u8 and routes are required)");
  RMEM_REQUIRE(Ho >= 1 && Wo >= 1 && (long)Ho * Wo <= kRouteMaxPixels, "rmem_route_labels: Ho and Wo must be positive, Ho * Wo at most 2^26");
  const int n = Ho * Wo;
  const int groups = (n + 3) / 4;
  hipLaunchKernelGGL(k_route_labels, dim3((groups + kRouteThreads - 1) / kRouteThreads, rows), dim3(kRouteThreads), 0, (hipStream_t)stream,
                     rows_u8, rows, n, Wo, routes);
  return rmem_check_launch("rmem_route_labels");
}
