// What the kernels that match boundary bit planes share (boundary.hip, boundary_pairs.hip): the tile of a match workgroup and the
// dilation of one 64-pixel word by a disk, from rows staged in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr int kRows = 16;             // match tile: rows
constexpr int kWords = 16;            // match tile: words per row (1024 pixels)
constexpr int kLdsWords = kWords + 2; // with one halo word on each side

// one-pixel horizontal dilation of the 192-bit row segment (l, c, r); bit 0 of a word is its leftmost pixel
__device__ __forceinline__ void widen1(uint64_t& l, uint64_t& c, uint64_t& r) {
  const uint64_t nl = l | (l << 1) | (l >> 1) | (c << 63);
  const uint64_t nc = c | (c << 1) | (l >> 63) | (c >> 1) | (r << 63);
  const uint64_t nr = r | (r << 1) | (c >> 63) | (r >> 1);
  l = nl; c = nc; r = nr;
}

// The word at tile position (ty, tx) of a plane dilated by the disk dx^2 + dy^2 <= radius^2.  rows: the plane's rows
// y0 - radius .. y0 + kRows - 1 + radius, kLdsWords words each (one halo word left and right), zero outside the image.
// A disk is the union over dy of horizontal runs of half-width h(dy) = floor(sqrt(r^2 - dy^2)), and h falls as |dy| grows, so with
// B_0 = row y and B_d = widen(B_{d-1}, h(d-1) - h(d)) | row(y - d) | row(y + d), B_r is the dilated row.  The edge error of the
// (left, centre, right) triple creeps inwards one bit per widening and never reaches the centre word while radius <= 63.
__device__ __forceinline__ uint64_t dilated_word(const uint64_t* rows, int ty, int tx, int radius) {
  const uint64_t* p = rows + (ty + radius) * kLdsWords + tx;
  uint64_t l = p[0], c = p[1], r = p[2];
  const int r2 = radius * radius;
  int h = radius;
  for (int d = 1; d <= radius; ++d) {
    while (h * h + d * d > r2) { widen1(l, c, r); --h; }
    const uint64_t* a = p - d * kLdsWords;
    const uint64_t* b = p + d * kLdsWords;
    l |= a[0] | b[0];
    c |= a[1] | b[1];
    r |= a[2] | b[2];
  }
  return c;
}
}  // namespace
