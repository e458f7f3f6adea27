// Exact Euclidean distance transform of uint8 label stacks and the peaks of a distance map (include/rmem.h: rmem_label_edt,
// rmem_label_edt_at, rmem_label_edt_peaks; distance.py, surface.py).  Squared distances between pixel centres as int32, integers
// only, no float anywhere.  Element-type agnostic (uint8 in, int32 out): built once.
//
// A SITE of pixel p is what p's distance is measured to: in the "other" mode (value = -1) a pixel of the frame that holds another
// value than p, and with `border` the first pixel outside the frame; in the "to value" mode the pixels that hold `value`.
// Separable, two passes (label_sep.h holds what they share with label_nearest.hip, the row pass' scan included):
//
//   k_edt_cols   One thread per column, 64 columns per workgroup: consecutive lanes read consecutive bytes of a row.  A sweep down
//                the column and one up keep the vertical distance to the last site met, g[y][x] = the smaller of the two as 16
//                bits, kNone where the column holds no site.  Other mode: the last site above is the end of the run of equal
//                values the pixel lies in (distance 1 where the value changes), the frame's edge with border.
//   k_edt_rows   One workgroup per row.  The row's labels and g go to LDS (50 KB at W = 16384, summaries included), then a thread
//                takes pixels x = t, t + 256, ...: d2(x) = min over x' of (x - x')^2 + f(x'), f = g^2 where the row holds p's value
//                at x' (to value: everywhere) and 0 at the first pixel of another value on either side, where that side ends.
//                label_sep.h's outward scan under EdtRule: it stops when dx^2 >= the best so far, so its length is bounded by the
//                root of the result, not by W.  Stride-1 LDS reads.  A segment keeps a summary in LDS (its smallest g; the value
//                its pixels share, if they do): a rest whose summary says that it cannot win -- no pixel of another value,
//                dx^2 + (smallest g)^2 not below the best so far -- is skipped in one step, so columns without a site and flat
//                stretches of g cost a look per 32 pixels.  A row that holds no site at all (one value, every g none; known from
//                a workgroup-wide OR while the row is loaded) is filled with the sentinel without a scan.
//   k_edt_rows_at
//                The to-value row pass at the pixels with keys == key alone (rmem_label_edt_at): a row without a key
//                pixel leaves before it reads g, in the others a thread per pixel skips the pixels without the key.
//   k_peaks_init, k_peaks, k_peaks_table
//                keys[f][v] = max over the pixels of frame f with key v of (d2 << 32) | (2^32 - 1 - flat index): the largest
//                distance, and among equals the first pixel in raster order.  A table per workgroup in LDS (64-bit integer max),
//                merged with one global 64-bit max per value the workgroup met; integers only, so arrival order does not matter.
//                The last launch unpacks the keys into (d2, index), (-1, -1) where the key is still 0 (no pixel).
//
// No kernel waits for another workgroup, every loop is bounded by H or W, nothing is indexed beyond [0, H) x [0, W).
#include "label_sep.h"
#include "../../include/rmem.h"

namespace {
constexpr int kNone = 0xffff;                      // g: no site in this column (a real g is at most kMaxSide)
constexpr int kMixed = 0x100;                      // a segment's value: its pixels differ
static_assert(2 * kMaxSide * kMaxSide < (1 << 30) + 1 && kMaxSide < kNone, "distance range");

__global__ __launch_bounds__(kColThreads) void k_edt_cols(const unsigned char* __restrict__ labels, int H, int W, int value, int border,
                                                          unsigned short* __restrict__ g) {
  const int x = blockIdx.x * kColThreads + threadIdx.x;
  if (x >= W) return;
  const size_t frame = (size_t)blockIdx.y * H * W;
  const unsigned char* L = labels + frame + x;
  unsigned short* G = g + frame + x;
  const bool other = value < 0;
  int d = border ? 0 : kNone, prev = -1;           // d: the distance of the row before; prev: its value
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    const int v = L[(size_t)y * W];
    const bool changed = other && y > 0 && v != prev;
    d = (!other && v == value) ? 0 : (changed ? 1 : (d == kNone ? kNone : d + 1));
    G[(size_t)y * W] = (unsigned short)d;
    prev = v;
  }
  d = border ? 0 : kNone;
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    const int v = L[(size_t)y * W];
    const bool changed = other && y < H - 1 && v != prev;
    d = (!other && v == value) ? 0 : (changed ? 1 : (d == kNone ? kNone : d + 1));
    const int down = G[(size_t)y * W];
    if (d < down) G[(size_t)y * W] = (unsigned short)d;
    prev = v;
  }
}

// label_sep.h's rule of the distance alone: best = min over the columns q of dx^2 + g(q)^2.  Only a strictly smaller distance
// improves it, so what can at most equal it is left out: >= in far and idle (NearestRule, which breaks ties by index, has >).
// kOther: the other-value mode, where a side ends at its first pixel of another value than `me`, at distance dx^2; the to-value
// mode reads neither sl nor suni.  A compile-time parameter: as a run-time member it keeps the mode's tests inside the scan's
// loops, which was measured slower in both modes.
template <bool kOther>
struct EdtRule {
  const unsigned short *sg, *smin, *suni;          // the row's g; per segment its smallest g and the value its pixels share
  const unsigned char* sl;                         // the row's labels
  int me, best;
  __device__ __forceinline__ bool far(int dx2) const { return dx2 >= best; }
  __device__ __forceinline__ bool idle(int k, int dx2) const {
    const int m = smin[k];
    return (m == kNone || dx2 + m * m >= best) && (!kOther || suni[k] == me);
  }
  __device__ __forceinline__ bool visit(int q, int dx2) {
    if (kOther && sl[q] != me) {
      best = dx2;
      return false;
    }
    const int gq = sg[q];
    best = gq != kNone ? min(best, dx2 + gq * gq) : best;
    return true;
  }
};

// LDS of k_edt_rows: [wpad] the row's g, [nseg] the smallest g of a segment, [nseg] the value all its pixels hold (kMixed if they
// differ), 16 bits each, then [W] the row's labels
inline size_t edt_rows_lds(int W) { return (size_t)row_wpad(W) * 2 + (size_t)row_segments(W) * 4 + W; }

__global__ __launch_bounds__(kThreads) void k_edt_rows(const unsigned char* __restrict__ labels, const unsigned short* __restrict__ g, int H,
                                                       int W, int wpad, int value, int border, int* __restrict__ dist2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nseg = row_segments(W);
  unsigned short *sg = (unsigned short*)smem, *smin = sg + wpad, *suni = smin + nseg;
  unsigned char* sl = (unsigned char*)(suni + nseg);
  const int t = threadIdx.x;
  const size_t base = ((size_t)blockIdx.y * H + blockIdx.x) * W;
  const bool other = value < 0;
  const int first = labels[base];
  int any = 0;
  for (int x = t; x < W; x += kThreads) {
    const int l = labels[base + x], gg = g[base + x];
    sl[x] = (unsigned char)l;
    sg[x] = (unsigned short)gg;
    any |= (gg != kNone) | (other & (l != first));
  }
  any = __syncthreads_or(any);                     // the barrier too
  if (!any) {                                      // no site in this row's columns and none in the row: none in the frame
    for (int x = t; x < W; x += kThreads) dist2[base + x] = kSentinel;
    return;
  }
  for (int k = t; k < nseg; k += kThreads) {
    const int x0 = k * kSeg, x1 = min(x0 + kSeg, W);
    int m = kNone, u = sl[x0];
    for (int x = x0; x < x1; ++x) {
      m = min(m, (int)sg[x]);
      if (sl[x] != u) u = kMixed;
    }
    smin[k] = (unsigned short)m;
    suni[k] = (unsigned short)u;
  }
  __syncthreads();
  for (int x = t; x < W; x += kThreads) {
    const int g0 = sg[x];
    int best = g0 == kNone ? kSentinel : g0 * g0;
    if (other) {                                   // the same in every thread
      if (border) {
        const int e = min(x + 1, W - x);
        best = min(best, e * e);
      }
      EdtRule<true> r{sg, smin, suni, sl, sl[x], best};
      scan_outward(r, x, W);
      best = r.best;
    } else {
      EdtRule<false> r{sg, smin, nullptr, nullptr, 0, best};
      scan_outward(r, x, W);
      best = r.best;
    }
    dist2[base + x] = best;
  }
}

// ------------------------------------------------------------------------------------------------------ sampled row pass
// The to-value row pass at the pixels with keys == key alone (rmem_label_edt_at).  One workgroup per row.  It reads the row's keys
// first and leaves at once when none is the key (a workgroup-wide OR): such a row never reads g.  Otherwise the row's g and the
// segment summaries go to LDS as in k_edt_rows (33 KB at W = 16384), and a thread takes pixels x = t, t + 256, ... and skips those
// without the key, under EdtRule<false>, the to-value form.  Labels are not needed: a site is where g == 0.  Compacting the key pixels
// into a list first was measured and gained nothing on sparse keys.
// LDS of k_edt_rows_at: [wpad] the row's g, [nseg] the smallest g of a segment, 16 bits each
inline size_t edt_rows_at_lds(int W) { return (size_t)row_wpad(W) * 2 + (size_t)row_segments(W) * 2; }

__global__ __launch_bounds__(kThreads) void k_edt_rows_at(const unsigned short* __restrict__ g, const unsigned char* __restrict__ keys,
                                                          int H, int W, int wpad, int key, int* __restrict__ samples) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nseg = row_segments(W);
  unsigned short *sg = (unsigned short*)smem, *smin = sg + wpad;
  const int t = threadIdx.x;
  const size_t base = ((size_t)blockIdx.y * H + blockIdx.x) * W;
  int has = 0;
  for (int x = t; x < W; x += kThreads) has |= keys[base + x] == key;
  if (!__syncthreads_or(has)) return;              // the same in every thread
  int any = 0;
  for (int x = t; x < W; x += kThreads) {
    const int gg = g[base + x];
    sg[x] = (unsigned short)gg;
    any |= gg != kNone;
  }
  any = __syncthreads_or(any);                     // the barrier too
  for (int k = t; k < nseg; k += kThreads) {
    const int x0 = k * kSeg, x1 = min(x0 + kSeg, W);
    int mn = kNone;
    for (int x = x0; x < x1; ++x) mn = min(mn, (int)sg[x]);
    smin[k] = (unsigned short)mn;
  }
  __syncthreads();
  for (int x = t; x < W; x += kThreads) {
    if (keys[base + x] != key) continue;
    const int g0 = sg[x];
    EdtRule<false> r{sg, smin, nullptr, nullptr, 0, g0 == kNone ? kSentinel : g0 * g0};
    scan_outward(r, x, W, any);                    // no site in the frame: the sentinel without a scan
    samples[base + x] = r.best;
  }
}

// ------------------------------------------------------------------------------------------------------------------- peaks
__global__ __launch_bounds__(kThreads) void k_peaks_init(unsigned long long* __restrict__ keys) {
  keys[(size_t)blockIdx.x * 256 + threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kThreads) void k_peaks(const int* __restrict__ dist2, const unsigned char* __restrict__ keyv, int HW,
                                                    unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long tab[256];
  const int t = threadIdx.x, f = blockIdx.y;
  tab[t] = 0ull;
  __syncthreads();
  const int* D = dist2 + (size_t)f * HW;
  const unsigned char* K = keyv + (size_t)f * HW;
  for (int p = blockIdx.x * kThreads + t; p < HW; p += gridDim.x * kThreads) {
    const int v = K[p];
    const unsigned long long key = ((unsigned long long)(unsigned)D[p] << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
    // entries only grow: a stale read can only let through a max that changes nothing
    if (key > __hip_atomic_load(&tab[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(&tab[v], key);
  }
  __syncthreads();
  if (tab[t]) atomicMax(keys + (size_t)f * 256 + t, tab[t]);
}

__global__ __launch_bounds__(kThreads) void k_peaks_table(const unsigned long long* __restrict__ keys, int* __restrict__ table) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long key = keys[i];
  table[2 * i] = key ? (int)(unsigned)(key >> 32) : -1;
  table[2 * i + 1] = key ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : -1;
}
}  // namespace

extern "C" long long rmem_label_edt_workspace_bytes(int n, int H, int W) { return sep_workspace_bytes(n, H, W); }   // g

extern "C" int rmem_label_edt(const unsigned char* labels, int n, int H, int W, int value, int border, int* dist2, void* workspace,
                              long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(labels && dist2 && workspace, "rmem_label_edt: null pointer (labels, dist2 and workspace are required)");
  RMEM_REQUIRE_SEP_STACK("rmem_label_edt", n, H, W);
  RMEM_REQUIRE(value >= -1 && value <= 255, "rmem_label_edt: value must be -1 (every other value) or in 0..255");
  RMEM_REQUIRE(border == 0 || border == 1, "rmem_label_edt: border must be 0 or 1");
  RMEM_REQUIRE(!(value >= 0 && border), "rmem_label_edt: border must be 0 with a value (the frame's edge is no pixel of it)");
  RMEM_REQUIRE_SEP_WORKSPACE("rmem_label_edt", "rmem_label_edt_workspace_bytes", n, H, W, workspace, workspace_bytes);
  unsigned short* g = (unsigned short*)workspace;
  hipLaunchKernelGGL(k_edt_cols, dim3((W + kColThreads - 1) / kColThreads, n), dim3(kColThreads), 0, (hipStream_t)stream, labels, H, W, value,
                     border, g);
  hipLaunchKernelGGL(k_edt_rows, dim3(H, n), dim3(kThreads), edt_rows_lds(W), (hipStream_t)stream, labels, g, H, W, row_wpad(W), value,
                     border, dist2);
  return rmem_check_launch("rmem_label_edt");
}

extern "C" int rmem_label_edt_at(const unsigned char* labels, const unsigned char* keys, int n, int H, int W, int value, int key, int* samples,
                                 void* workspace, long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(labels && keys && samples && workspace, "rmem_label_edt_at: null pointer (labels, keys, samples and workspace are required)");
  RMEM_REQUIRE_SEP_STACK("rmem_label_edt_at", n, H, W);
  RMEM_REQUIRE(value >= 0 && value <= 255, "rmem_label_edt_at: value must be in 0..255");
  RMEM_REQUIRE(key >= 0 && key <= 255, "rmem_label_edt_at: key must be in 0..255");
  RMEM_REQUIRE_SEP_WORKSPACE("rmem_label_edt_at", "rmem_label_edt_workspace_bytes", n, H, W, workspace, workspace_bytes);
  unsigned short* g = (unsigned short*)workspace;
  hipLaunchKernelGGL(k_edt_cols, dim3((W + kColThreads - 1) / kColThreads, n), dim3(kColThreads), 0, (hipStream_t)stream, labels, H, W, value,
                     0, g);
  hipLaunchKernelGGL(k_edt_rows_at, dim3(H, n), dim3(kThreads), edt_rows_at_lds(W), (hipStream_t)stream, g, keys, H, W, row_wpad(W), key,
                     samples);
  return rmem_check_launch("rmem_label_edt_at");
}

extern "C" long long rmem_label_edt_peaks_workspace_bytes(int n) {
  if (n < 1 || n > kMaxFrames) return 0;
  return (long long)n * 256 * 8;                                   // one 64-bit key per frame and value
}

extern "C" int rmem_label_edt_peaks(const int* dist2, const unsigned char* keys, int n, int H, int W, int* table, void* workspace,
                                    long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(dist2 && keys && table && workspace, "rmem_label_edt_peaks: null pointer (dist2, keys, table and workspace are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_edt_peaks: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_edt_peaks: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(workspace_bytes >= rmem_label_edt_peaks_workspace_bytes(n),
               "rmem_label_edt_peaks: workspace too small (rmem_label_edt_peaks_workspace_bytes)");
  RMEM_REQUIRE(((uintptr_t)workspace & 7u) == 0, "rmem_label_edt_peaks: workspace must be 8-byte aligned");
  unsigned long long* k = (unsigned long long*)workspace;
  const int HW = H * W;
  hipLaunchKernelGGL(k_peaks_init, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, k);
  hipLaunchKernelGGL(k_peaks, dim3(blocks_per_frame(16L * HW, n), n), dim3(kThreads), 0, (hipStream_t)stream, dist2, keys, HW, k);
  hipLaunchKernelGGL(k_peaks_table, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, k, table);
  return rmem_check_launch("rmem_label_edt_peaks");
}
