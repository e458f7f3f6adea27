// Nearest-site feature transform of uint8 label stacks (include/rmem.h: rmem_label_nearest; distance.py: nearest, grow).  Where
// label_edt.hip says how far the nearest site is, this says WHICH pixel it is, and reads the label there.  Integers only, no
// atomics.  Element-type agnostic (uint8 in, int32 / uint8 out): built once.
//
// A SITE is a pixel whose value is in the set `sites` (256 bits).  index[p] = the flat index y * W + x of the site nearest to p by
// squared Euclidean distance between pixel centres, AMONG EQUALLY NEAR SITES THE ONE WITH THE SMALLEST FLAT INDEX; -1 where the
// frame holds no site within max_d2.  Separable, two passes:
//
//   k_nearest_cols  One thread per column, 64 columns per workgroup, as k_edt_cols.  It keeps the signed offset s = y_site - y of
//                   the nearest site of the pixel's own column as 16 bits, kNoSite where the column holds none.  The sweep down
//                   writes the offset to the last site above (<= 0); the sweep up replaces it only where the site below is
//                   STRICTLY nearer: of two equally near sites of a column the one above (the smaller index) stays.  So every
//                   column's candidate is the smallest-index nearest site of that column to row y.
//   k_nearest_rows  One workgroup per row.  The row's s and the smallest |s| of every segment of kSeg pixels go to LDS (33 KB at
//                   W = 16384); labels are not staged, a site is where s == 0.  A thread takes pixels x = t, t + 256, ... and
//                   keeps the lexicographic minimum of (d2, index) over the columns x': d2 = (x - x')^2 + s(x')^2, index =
//                   (y + s(x')) * W + x'.  label_sep.h's outward scan under NearestRule, whose bounds are both STRICT: a side ends
//                   only when dx^2 > the best d2, a segment's rest is skipped only when dx^2 + (its smallest |s|)^2 > the best
//                   d2, because a candidate at exactly the best d2 may still win on its index.  With a limit the scan starts at
//                   best = max_d2 and is never longer than its root.  taken[p] = labels[index[p]] where labels[p] is in `fill`
//                   and a site was found, else labels[p]: one byte read at the winner.  When only `taken` is asked for, pixels
//                   outside `fill` are copied without a scan and a row without a pixel in `fill` leaves before it reads s (a
//                   workgroup-wide OR); a row of a frame without a site (no column has one) is filled without a scan.
//
// The two sets are kernel arguments (eight 32-bit words each): no table on the device, no upload.  No kernel waits for another
// workgroup, every loop is bounded by H, W or a segment, nothing is indexed beyond [0, H) x [0, W).
#include "label_sep.h"
#include "../../include/rmem.h"

namespace {
constexpr int kNoSite = -32768;                    // s: no site in this column (0x8000); |s| <= kMaxSide - 1 fits 15 bits
constexpr int kNoMin = 0xffff;                     // a segment's smallest |s|: no site in any of its columns
constexpr int kMaxD2 = 1 << 30;                    // above every real squared distance
static_assert(2 * (kMaxSide - 1) * (kMaxSide - 1) < kMaxD2 && kMaxSide - 1 < -kNoSite, "distance range");

struct Bits256 {
  unsigned w[8];
};
__device__ __forceinline__ bool in_set(const Bits256& b, int v) { return (b.w[v >> 5] >> (v & 31)) & 1u; }

__global__ __launch_bounds__(kColThreads) void k_nearest_cols(const unsigned char* __restrict__ labels, int H, int W, Bits256 sites,
                                                              short* __restrict__ s) {
  const int x = blockIdx.x * kColThreads + threadIdx.x;
  if (x >= W) return;
  const size_t frame = (size_t)blockIdx.y * H * W;
  const unsigned char* L = labels + frame + x;
  short* S = s + frame + x;
  int ys = -1;                                     // the row of the last site met, -1: none yet
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    if (in_set(sites, L[(size_t)y * W])) ys = y;
    S[(size_t)y * W] = (short)(ys < 0 ? kNoSite : ys - y);
  }
  ys = -1;
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    const int down = S[(size_t)y * W];
    if (down == 0) ys = y;                         // a site: what the sweep down wrote there
    const int up = ys - y;
    if (ys >= 0 && (down == kNoSite || up < -down)) S[(size_t)y * W] = (short)up;   // strictly nearer only: above wins a tie
  }
}

// label_sep.h's rule of the nearest site: (best, bidx) = the lexicographic minimum over the columns q of (d2, index), d2 = dx^2 +
// s(q)^2, index = (y + s(q)) * W + q.  A candidate at exactly the best d2 may still win on its index, so only what is strictly
// farther is left out: > in far and idle (EdtRule, which keeps the distance alone, has >=).  bidx INT_MAX: nothing found yet;
// any real index beats it on a tie.
struct NearestRule {
  const short* ss;                                 // the row's s
  const unsigned short* smin;                      // per segment its smallest |s|
  int y, W, best, bidx;
  __device__ __forceinline__ bool far(int dx2) const { return dx2 > best; }
  __device__ __forceinline__ bool idle(int k, int dx2) const {
    const int m = smin[k];
    return m == kNoMin || dx2 + m * m > best;
  }
  __device__ __forceinline__ bool visit(int q, int dx2) {
    const int sq = ss[q], d2 = dx2 + sq * sq, idx = (y + sq) * W + q;
    if (sq != kNoSite && (d2 < best || (d2 == best && idx < bidx))) {
      best = d2;
      bidx = idx;
    }
    return true;
  }
};

// LDS of k_nearest_rows: [wpad] the row's s, [nseg] the smallest |s| of a segment, 16 bits each
inline size_t nearest_rows_lds(int W) { return (size_t)row_wpad(W) * 2 + (size_t)row_segments(W) * 2; }

__global__ __launch_bounds__(kThreads) void k_nearest_rows(const unsigned char* __restrict__ labels, const short* __restrict__ s, int H, int W,
                                                           int wpad, Bits256 fill, int max_d2, int* __restrict__ index,
                                                           int* __restrict__ dist2, unsigned char* __restrict__ taken) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nseg = row_segments(W);
  short* ss = (short*)smem;
  unsigned short* smin = (unsigned short*)(ss + wpad);
  const int t = threadIdx.x, y = blockIdx.x;
  const size_t frame = (size_t)blockIdx.y * H * W, base = frame + (size_t)y * W;
  const bool maps = index || dist2;                // the same in every thread
  if (!maps) {                                     // taken alone: a row without a pixel to fill is a copy
    int has = 0;
    for (int x = t; x < W; x += kThreads) has |= in_set(fill, labels[base + x]);
    if (!__syncthreads_or(has)) {
      for (int x = t; x < W; x += kThreads) taken[base + x] = labels[base + x];
      return;
    }
  }
  int any = 0;
  for (int x = t; x < W; x += kThreads) {
    const int sx = s[base + x];
    ss[x] = (short)sx;
    any |= sx != kNoSite;
  }
  any = __syncthreads_or(any);                     // the barrier too
  if (!any) {                                      // no column of the frame holds a site
    for (int x = t; x < W; x += kThreads) {
      if (index) index[base + x] = -1;
      if (dist2) dist2[base + x] = kSentinel;
      if (taken) taken[base + x] = labels[base + x];
    }
    return;
  }
  for (int k = t; k < nseg; k += kThreads) {
    const int x0 = k * kSeg, x1 = min(x0 + kSeg, W);
    int m = kNoMin;
    for (int x = x0; x < x1; ++x) {
      const int sx = ss[x];
      if (sx != kNoSite) m = min(m, abs(sx));
    }
    smin[k] = (unsigned short)m;
  }
  __syncthreads();
  for (int x = t; x < W; x += kThreads) {
    const int me = labels[base + x];
    const bool fills = taken && in_set(fill, me);
    if (!maps && !fills) {
      taken[base + x] = (unsigned char)me;
      continue;
    }
    NearestRule r{ss, smin, y, W, max_d2 < 0 ? kSentinel : max_d2, INT_MAX};
    r.visit(x, 0);                                 // the pixel's own column
    scan_outward(r, x, W);
    const bool found = r.bidx != INT_MAX;
    if (index) index[base + x] = found ? r.bidx : -1;
    if (dist2) dist2[base + x] = found ? r.best : kSentinel;
    if (taken) taken[base + x] = (fills && found) ? labels[frame + r.bidx] : (unsigned char)me;
  }
}
}  // namespace

extern "C" long long rmem_label_nearest_workspace_bytes(int n, int H, int W) { return sep_workspace_bytes(n, H, W); }   // s

extern "C" int rmem_label_nearest(const unsigned char* labels, int n, int H, int W, const unsigned int site_bits[8],
                                  const unsigned int fill_bits[8], int max_d2, int* index, int* dist2, unsigned char* taken, void* workspace,
                                  long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(labels && site_bits && workspace, "rmem_label_nearest: null pointer (labels, site_bits and workspace are required)");
  RMEM_REQUIRE(index || dist2 || taken, "rmem_label_nearest: no output (at least one of index, dist2 and taken is required)");
  RMEM_REQUIRE(taken != labels, "rmem_label_nearest: taken must not be labels (labels are read at the nearest site while taken is written)");
  RMEM_REQUIRE_SEP_STACK("rmem_label_nearest", n, H, W);
  RMEM_REQUIRE(max_d2 >= -1 && max_d2 <= kMaxD2, "rmem_label_nearest: max_d2 must be -1 (no limit) or in 0..2^30");
  RMEM_REQUIRE_SEP_WORKSPACE("rmem_label_nearest", "rmem_label_nearest_workspace_bytes", n, H, W, workspace, workspace_bytes);
  Bits256 sites, fill;
  for (int i = 0; i < 8; ++i) {
    sites.w[i] = site_bits[i];
    fill.w[i] = fill_bits ? fill_bits[i] : 0xffffffffu;
  }
  short* s = (short*)workspace;
  hipLaunchKernelGGL(k_nearest_cols, dim3((W + kColThreads - 1) / kColThreads, n), dim3(kColThreads), 0, (hipStream_t)stream, labels, H, W, sites,
                     s);
  hipLaunchKernelGGL(k_nearest_rows, dim3(H, n), dim3(kThreads), nearest_rows_lds(W), (hipStream_t)stream, labels, s, H, W, row_wpad(W), fill,
                     max_d2, index, dist2, taken);
  return rmem_check_launch("rmem_label_nearest");
}
