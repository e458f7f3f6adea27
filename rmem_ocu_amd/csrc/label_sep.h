// What the separable transforms of uint8 label stacks share (label_edt.hip, label_nearest.hip): a column pass leaves 16 bits per
// pixel in a workspace, a row pass stages its row of them in LDS with one summary per segment of kSeg pixels and scans outward
// from every pixel.  Here: the limits, the workspace and row geometry, the refusals of the entry points, and the outward scan.
#pragma once
#include <limits.h>
#include "label_wave.h"

namespace {
constexpr int kMaxSide = 16384;                    // a vertical distance fits 15 bits, every real squared distance is below 2^30
constexpr int kSentinel = INT_MAX;                 // dist2: no site in this frame
constexpr int kColThreads = 64;                    // columns of a workgroup of a column pass, a thread each
constexpr int kSeg = 32;                           // pixels of a row that share one summary in a row pass

__host__ __device__ constexpr int row_segments(int W) { return (W + kSeg - 1) / kSeg; }
inline int row_wpad(int W) { return (W + 7) & ~7; }   // 16-bit entries of a row in LDS: what follows them starts on 16 bytes

inline bool sep_geometry_ok(int n, int H, int W) { return stack_geometry_ok(n, H, W) && H <= kMaxSide && W <= kMaxSide; }
// the column pass' 16 bits per pixel, rounded up to 16 bytes; 0 for a stack that is refused
inline long long sep_workspace_bytes(int n, int H, int W) { return sep_geometry_ok(n, H, W) ? ((long long)n * H * W * 2 + 15) & ~15LL : 0; }

// The refusals every entry point of a separable transform shares, before and after its own: `fn` and `sizer` (the exported
// function that states the workspace size) are string literals.
#define RMEM_REQUIRE_SEP_STACK(fn, n, H, W)                                                                      \
  RMEM_REQUIRE((n) >= 1 && (n) <= kMaxFrames, fn ": n must be in 1..65535");                                     \
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), fn ": H and W must be positive, H * W at most 2^26");                 \
  RMEM_REQUIRE((H) <= kMaxSide && (W) <= kMaxSide, fn ": H and W must be at most 16384")
#define RMEM_REQUIRE_SEP_WORKSPACE(fn, sizer, n, H, W, workspace, workspace_bytes)                               \
  RMEM_REQUIRE((workspace_bytes) >= sep_workspace_bytes(n, H, W), fn ": workspace too small (" sizer ")");       \
  RMEM_REQUIRE(((uintptr_t)(workspace) & 3u) == 0, fn ": workspace must be 4-byte aligned")

// ------------------------------------------------------------------------------------------------------- the outward scan
// The row pass of the pixel at column x: the minimum over the columns q of the row of a key that grows with dx^2 = (q - x)^2.
// The two sides take turns, the rest of a segment at a time, so the nearer side tightens the bound of the other.  What the key
// is, and when it can no longer improve, is the RULE's: a struct that holds the LDS pointers and the running result, with
//   bool far(dx2)       nothing at this horizontal distance or beyond can matter: the side ends;
//   bool idle(k, dx2)   segment k's summary says that its rest, dx2 or more away, cannot matter: it is skipped in one step;
//   bool visit(q, dx2)  takes column q into the result; false: this side is done.
// far and idle are where a rule decides between >= and > against its best: see EdtRule and NearestRule.

// the rest of the segment the cursor q stands in, towards `end` (inclusive) in steps of `step`; false: this side is done
template <class Rule>
__device__ __forceinline__ bool scan_rest(Rule& r, int x, int q, int end, int step) {
  for (;; q += step) {
    const int dx = (q - x) * step;
    if (r.far(dx * dx) || !r.visit(q, dx * dx)) return false;
    if (q == end) return true;
  }
}

// one turn of the side that walks in steps of `step` (-1 or 1) with its cursor at q; false: this side is done
template <class Rule>
__device__ __forceinline__ bool scan_turn(Rule& r, int x, int W, int& q, int step) {
  const int dx = (q - x) * step, k = q / kSeg;
  if (r.far(dx * dx)) return false;
  const int end = step < 0 ? k * kSeg : min(k * kSeg + kSeg, W) - 1;
  const bool on = r.idle(k, dx * dx) || scan_rest(r, x, q, end, step);
  q = end + step;
  return on && (step < 0 ? q >= 0 : q < W);
}

// go false: no scan at all (the caller knows that the row holds nothing to find)
template <class Rule>
__device__ __forceinline__ void scan_outward(Rule& r, int x, int W, bool go = true) {
  int ql = x - 1, qr = x + 1;
  bool left = go && ql >= 0, right = go && qr < W;
  while (left || right) {
    if (left) left = scan_turn(r, x, W, ql, -1);
    if (right) right = scan_turn(r, x, W, qr, 1);
  }
}
}  // namespace
