// Connected components of uint8 label stacks (include/rmem.h: rmem_label_components, rmem_label_component_stats, rmem_label_clean):
// the pieces of every value of every frame, their statistics and the clean-up rule on top (components.py).  Element-type agnostic
// (uint8 in, int32 / uint8 out): built once.
//
// Union-find in which the smaller index always wins, so a set's representative is its first pixel in raster order and the result
// is the same whatever the schedule.  Separate launches; no kernel waits for or spins on another workgroup, every loop that walks
// parents carries a bound, and reaching one sets a bit of the caller's status word (bit 0: union, bit 1: find) -- a bug, not a
// condition.
//
//   k_cc_tile     One workgroup per tile of kTH x kTW pixels.  The tile's bytes go to LDS: per tile row the 16-byte pieces that
//                 cover it, one piece per lane as one 16-byte load where the piece lies inside the stack, single bytes otherwise
//                 (a frame and a row may start at any byte).  A thread owns 8 pixels of a row: their parents start at the first
//                 pixel of the run inside those 8, then it unites what the runs leave open (the left neighbour of its first
//                 pixel, up, and for 8 the two upper diagonals; a link that the pixel to the left makes anyway is skipped) with
//                 LDS atomicMin.  Last, every pixel's parent is written as the GLOBAL flat index of its tile-local root, 64
//                 consecutive ints per wave.
//   k_cc_seam     Pixels of a tile's first row and first column unite with their neighbours in other tiles (up, left, for 8 the
//                 upper diagonals and, from the first column, the lower-left one) in global memory: find walks parents (relaxed
//                 agent-scope loads; parents only decrease, so an old value is an ancestor still), atomicMin(&parent[larger root],
//                 smaller) links, and only the value the atomic returns decides: if it is not the root that was expected, the
//                 union carries on from it.
//   k_cc_flatten  roots[p] = find(p), in place.
//   k_cc_init, k_cc_stats
//                 (0, 256, -1, 0) everywhere and (0, 0, -1) in the table first.  Then a lane takes 4 consecutive pixels, a wave
//                 256: for every distinct root among them (picked from the first lane that has pixels left) the lanes' partial
//                 area, neighbour minimum / maximum and border bit are reduced over the wave and four lanes make one integer
//                 atomic each (add / min / max / or) -- none where the wave has nothing to say (no differing neighbour, no border
//                 pixel).  A wave takes one such piece, so at most one atomic per (wave, root, statistic) reaches memory.
//   k_cc_table_count, k_cc_table_root
//                 Per value: the number of roots and the largest area (LDS tables per workgroup, flushed with add / max), then,
//                 in a second launch, the smallest root whose area is that maximum (unsigned min over -1).
//   k_cc_clean    dst from src, roots, stats and table; 16 pixels per lane, 16-byte stores where dst allows, single bytes at head
//                 and tail; every byte is read and written by the same thread, and read first (dst == src is allowed).  A lane
//                 keeps the last root's decision, label maps being long runs of one root.
#include <limits.h>
#include "label_wave.h"
#include "../../include/rmem.h"

namespace {
constexpr int kTH = 32, kTW = 64;                 // the tile; kTW * kTH = 8 pixels per thread
constexpr int kSeg = 8;                           // pixels of one row a thread owns in k_cc_tile
constexpr int kPieces = kTW / 16 + 1;             // 16-byte pieces that can cover a tile row starting at any byte
constexpr int kStatusUnion = 1, kStatusFind = 2;
static_assert(kTH * kTW == kThreads * kSeg && kTW % kSeg == 0 && kTH * kPieces <= kThreads, "tile geometry");
constexpr int kSeamThreads = 128;                 // the first row and the rest of the first column of a tile
static_assert(kTW + kTH - 1 <= kSeamThreads, "seam geometry");

// ------------------------------------------------------------------------------------------------------------------ in LDS
__device__ __forceinline__ int lds_find(int* par, int x, int* status) {
  for (int it = 0; it <= kTH * kTW; ++it) {
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
  atomicOr(status, kStatusFind);
  return -1;
}
__device__ __forceinline__ void lds_union(int* par, int a, int b, int* status) {
  a = lds_find(par, a, status);
  b = lds_find(par, b, status);
  if (a < 0 || b < 0) return;
  for (int it = 0; it < kTH * kTW + 64; ++it) {
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;                          // a was a root and hangs below b now
    a = old;                                       // a had a parent: that one and b remain to be united
  }
  atomicOr(status, kStatusUnion);
}

__global__ __launch_bounds__(kThreads) void k_cc_tile(const unsigned char* __restrict__ labels, size_t stack_bytes, int H, int W, int tiles_x,
                                                      int conn8, int* __restrict__ roots, int* __restrict__ status) {
  __shared__ int par[kTH * kTW];
  __shared__ __attribute__((aligned(16))) unsigned char val[kTH][kTW];
  const int t = threadIdx.x, f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * kTH, x0 = tx * kTW;
  const int th = min(kTH, H - y0), tw = min(kTW, W - x0);
  const size_t HW = (size_t)H * W;
  const unsigned char* frame = labels + (size_t)f * HW;
  if (t < kTH * kPieces) {                                         // the tile's bytes: one 16-byte piece of one row per lane
    const int row = t / kPieces, k = t - row * kPieces;
    if (row < th) {
      const unsigned char* a = frame + (size_t)(y0 + row) * W + x0;                // the row's first byte
      const unsigned char* c = a - ((uintptr_t)a & 15u) + 16 * k;                   // this lane's piece (may begin before a)
      const long first = c - a;                                                     // tile column of the piece's byte 0
      if (first < tw) {
        if (c >= labels && c + 16 <= labels + stack_bytes) {
          const uint4 w = *(const uint4*)c;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const long lx = first + j;
            if (lx >= 0 && lx < tw) val[row][lx] = (unsigned char)byte_at(w, j);
          }
        } else {
          for (int j = 0; j < 16; ++j) {
            const long lx = first + j;
            if (lx >= 0 && lx < tw) val[row][lx] = c[j];
          }
        }
      }
    }
  }
  __syncthreads();
  const int ly = t / (kTW / kSeg), lx0 = (t - ly * (kTW / kSeg)) * kSeg;
  const bool live = ly < th && lx0 < tw;
  int v[kSeg];
  if (live) {                                                      // parents: the first pixel of the run inside the thread's 8
    int start = ly * kTW + lx0;
#pragma unroll
    for (int j = 0; j < kSeg; ++j) {
      v[j] = lx0 + j < tw ? (int)val[ly][lx0 + j] : -1;
      if (j > 0 && v[j] != v[j - 1]) start = ly * kTW + lx0 + j;
      if (lx0 + j < tw) par[ly * kTW + lx0 + j] = start;
    }
  }
  __syncthreads();
  if (live) {
    int left = lx0 > 0 ? (int)val[ly][lx0 - 1] : -1;              // the value to the left of pixel j, and above it
    int upleft = ly > 0 && lx0 > 0 ? (int)val[ly - 1][lx0 - 1] : -1;
#pragma unroll
    for (int j = 0; j < kSeg; ++j) {
      const int lx = lx0 + j;
      if (lx >= tw) break;
      const int i = ly * kTW + lx, me = v[j];
      const int up = ly > 0 ? (int)val[ly - 1][lx] : -1;
      const int upright = ly > 0 && lx + 1 < tw ? (int)val[ly - 1][lx + 1] : -1;
      if (j == 0 && left == me) lds_union(par, i, i - 1, status);
      // up: where left and up-left hold the value too, the pixel to the left makes the link (or the one to its left, ...)
      if (up == me && !(left == me && upleft == me)) lds_union(par, i, i - kTW, status);
      if (conn8) {
        if (upleft == me && up != me && left != me) lds_union(par, i, i - kTW - 1, status);   // else up or left reaches it
        if (upright == me && up != me) lds_union(par, i, i - kTW + 1, status);                // else up's run reaches it
      }
      left = me;
      upleft = up;
    }
  }
  __syncthreads();
  int* out = roots + (size_t)f * HW;
#pragma unroll
  for (int k = 0; k < kSeg; ++k) {                                 // 64 consecutive ints per wave
    const int i = k * kThreads + t, row = i / kTW, lx = i - row * kTW;
    if (row < th && lx < tw) {
      const int r = lds_find(par, i, status);
      if (r >= 0) {
        const int ry = r / kTW;
        out[(size_t)(y0 + row) * W + x0 + lx] = (y0 + ry) * W + x0 + (r - ry * kTW);
      } else {
        out[(size_t)(y0 + row) * W + x0 + lx] = (y0 + row) * W + x0 + lx;   // never: the status bit is set; a root of its own keeps later walks finite
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------- in global memory
__device__ __forceinline__ int g_find(int* par, int x, int bound, int* status) {
  for (int it = 0; it <= bound; ++it) {
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    if ((unsigned)p >= (unsigned)bound) break;     // never: not a parent the tile pass wrote
    x = p;
  }
  atomicOr(status, kStatusFind);
  return -1;
}
__device__ __forceinline__ void g_union(int* par, int a, int b, int HW, int* status) {
  a = g_find(par, a, HW, status);
  b = g_find(par, b, HW, status);
  if (a < 0 || b < 0) return;
  for (int it = 0; it < HW + 64; ++it) {
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
  atomicOr(status, kStatusUnion);
}

__global__ __launch_bounds__(kSeamThreads) void k_cc_seam(const unsigned char* __restrict__ labels, int H, int W, int tiles_x, int conn8, int* roots,
                                                 int* __restrict__ status) {
  const int t = threadIdx.x, f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ly = t < kTW ? 0 : t - kTW + 1, lx = t < kTW ? t : 0;    // the first row, then the rest of the first column
  if (ly >= kTH) return;
  const int y = ty * kTH + ly, x = tx * kTW + lx;
  if (y >= H || x >= W) return;
  const bool top = ly == 0 && y > 0, side = lx == 0 && x > 0;
  if (!top && !side) return;
  const int HW = H * W;
  const unsigned char* L = labels + (size_t)f * HW;
  int* par = roots + (size_t)f * HW;
  const int p = y * W + x, me = L[p];
  if (top && L[p - W] == me) g_union(par, p, p - W, HW, status);
  if (side && L[p - 1] == me) g_union(par, p, p - 1, HW, status);
  if (conn8) {
    if (y > 0 && x > 0 && L[p - W - 1] == me) g_union(par, p, p - W - 1, HW, status);
    if (top && x + 1 < W && L[p - W + 1] == me) g_union(par, p, p - W + 1, HW, status);
    if (side && y + 1 < H && L[p + W - 1] == me) g_union(par, p, p + W - 1, HW, status);
  }
}

__global__ __launch_bounds__(kThreads) void k_cc_flatten(int HW, int* roots, int* __restrict__ status) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  int* par = roots + (size_t)blockIdx.y * HW;
  const int r = g_find(par, p, HW, status);
  if (r >= 0) par[p] = r;
}

// -------------------------------------------------------------------------------------------------------------- statistics
__global__ __launch_bounds__(kThreads) void k_cc_init(int* __restrict__ stats, int HW4, int* __restrict__ table) {
  const int i = blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y;
  if (i < HW4) {
    const int k = i & 3;
    stats[(size_t)f * HW4 + i] = k == 1 ? 256 : (k == 2 ? -1 : 0);
  }
  if (i < 256 * 3) table[(size_t)f * 768 + i] = i % 3 == 2 ? -1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_cc_stats(const unsigned char* __restrict__ labels, const int* __restrict__ roots, int H, int W,
                                                       int conn8, int* __restrict__ stats) {
  const int t = threadIdx.x, lane = t & 63, f = blockIdx.y;
  const int HW = H * W;
  const unsigned char* L = labels + (size_t)f * HW;
  const int* R = roots + (size_t)f * HW;
  int* S = stats + (size_t)f * HW * 4;
  const int p0 = (blockIdx.x * kThreads + t) * 4;
  int root[4], mn[4], mx[4], bd[4];
  unsigned rem = 0;
  if (p0 < HW) {
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + j;
      root[j] = 0; mn[j] = 256; mx[j] = -1; bd[j] = 0;
      if (p < HW) {
        root[j] = R[p];
        if ((unsigned)root[j] < (unsigned)HW) rem |= 1u << j;      // anything else is not a root of rmem_label_components: no entry
        const int me = L[p];
        const bool u = y > 0, d = y + 1 < H, l = x > 0, r = x + 1 < W;
        bd[j] = !(u && d && l && r);
        int nb;
#define RMEM_CC_NB(cond, q)                                      \
  if (cond) {                                                     \
    nb = L[q];                                                    \
    if (nb != me) { mn[j] = min(mn[j], nb); mx[j] = max(mx[j], nb); } \
  }
        RMEM_CC_NB(u, p - W)
        RMEM_CC_NB(d, p + W)
        RMEM_CC_NB(l, p - 1)
        RMEM_CC_NB(r, p + 1)
        if (conn8) {
          RMEM_CC_NB(u && l, p - W - 1)
          RMEM_CC_NB(u && r, p - W + 1)
          RMEM_CC_NB(d && l, p + W - 1)
          RMEM_CC_NB(d && r, p + W + 1)
        }
#undef RMEM_CC_NB
        if (++x == W) { x = 0; ++y; }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { root[j] = 0; mn[j] = 256; mx[j] = -1; bd[j] = 0; }
  }
  for (;;) {                                                       // whole waves: one distinct root per round
    const uint64_t busy = __ballot(rem != 0);
    if (!busy) break;
    const int k = rem ? __builtin_ctz(rem) : 0;
    const int cand = k == 0 ? root[0] : (k == 1 ? root[1] : (k == 2 ? root[2] : root[3]));
    const int r0 = __builtin_amdgcn_readlane(cand, __builtin_ctzll(busy));
    int a = 0, lo = 256, hi = -1, b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (((rem >> j) & 1u) && root[j] == r0) {
        ++a; lo = min(lo, mn[j]); hi = max(hi, mx[j]); b |= bd[j];
        rem &= ~(1u << j);
      }
    }
    const int area = wave_isum(a);
    const bool any_nb = __ballot(hi >= 0) != 0, any_bd = __ballot(b != 0) != 0;
    if (any_nb) { lo = wave_imin(lo); hi = wave_imax(hi); }
    int* o = S + (size_t)r0 * 4;
    if (lane == 0) atomicAdd(o + 0, area);
    else if (lane == 1) { if (any_nb) atomicMin(o + 1, lo); }
    else if (lane == 2) { if (any_nb) atomicMax(o + 2, hi); }
    else if (lane == 3) { if (any_bd) atomicOr(o + 3, 1); }
  }
}

// the number of components and the largest area of every value
__global__ __launch_bounds__(kThreads) void k_cc_table_count(const unsigned char* __restrict__ labels, const int* __restrict__ roots, int HW,
                                                             const int* __restrict__ stats, int* __restrict__ table) {
  __shared__ int cnt[256], best[256];
  const int t = threadIdx.x, f = blockIdx.y;
  cnt[t] = 0; best[t] = 0;
  __syncthreads();
  const unsigned char* L = labels + (size_t)f * HW;
  const int* R = roots + (size_t)f * HW;
  const int* S = stats + (size_t)f * HW * 4;
  for (int p = blockIdx.x * kThreads + t; p < HW; p += gridDim.x * kThreads) {
    if (R[p] == p) {
      const int v = L[p];
      atomicAdd(&cnt[v], 1);
      atomicMax(&best[v], S[(size_t)p * 4]);
    }
  }
  __syncthreads();
  if (cnt[t]) {
    int* o = table + ((size_t)f * 256 + t) * 3;
    atomicAdd(o + 0, cnt[t]);
    atomicMax(o + 1, best[t]);
  }
}

// the smallest root among the largest components of every value (unsigned: the table's -1 is "none yet")
__global__ __launch_bounds__(kThreads) void k_cc_table_root(const unsigned char* __restrict__ labels, const int* __restrict__ roots, int HW,
                                                            const int* __restrict__ stats, int* table) {
  __shared__ unsigned first[256];
  const int t = threadIdx.x, f = blockIdx.y;
  first[t] = 0xffffffffu;
  __syncthreads();
  const unsigned char* L = labels + (size_t)f * HW;
  const int* R = roots + (size_t)f * HW;
  const int* S = stats + (size_t)f * HW * 4;
  int* T = table + (size_t)f * 768;
  for (int p = blockIdx.x * kThreads + t; p < HW; p += gridDim.x * kThreads) {
    if (R[p] == p) {
      const int v = L[p];
      if (S[(size_t)p * 4] == T[v * 3 + 1]) atomicMin(&first[v], (unsigned)p);
    }
  }
  __syncthreads();
  if (first[t] != 0xffffffffu) atomicMin((unsigned*)(T + t * 3 + 2), first[t]);
}

// ------------------------------------------------------------------------------------------------------------------- apply
struct CleanRule {
  int max_hole, max_sprinkle, keep_largest;
};

__device__ __forceinline__ int clean_one(int v, int r, const int* __restrict__ S, const int* __restrict__ T, int HW, CleanRule rule) {
  if ((unsigned)r >= (unsigned)HW) return v;       // not a root of rmem_label_components: the pixel stays
  const int* s = S + (size_t)r * 4;
  const int area = s[0], lo = s[1], hi = s[2];
  if (v == 0) return area <= rule.max_hole && s[3] == 0 && lo == hi ? lo : 0;
  if (area <= rule.max_sprinkle || (rule.keep_largest && r != T[v * 3 + 2])) return lo == hi ? lo : 0;
  return v;
}

__device__ __forceinline__ uint32_t clean4(uint32_t w, int r0, int r1, int r2, int r3, int& last_r, int& last_o,
                                           const int* __restrict__ S, const int* __restrict__ T, int HW, CleanRule rule) {
  const int rs[4] = {r0, r1, r2, r3};
  uint32_t o = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = (int)((w >> (8 * j)) & 0xffu);
    if (rs[j] != last_r) {                                         // a root holds one value: (root) decides
      last_r = rs[j];
      last_o = clean_one(v, rs[j], S, T, HW, rule);
    }
    o |= (uint32_t)last_o << (8 * j);
  }
  return o;
}

// src and dst may be the same frame: every byte is read and written by the same thread, and read first.
__global__ __launch_bounds__(kThreads) void k_cc_clean(const unsigned char* src, unsigned char* dst, const int* __restrict__ roots,
                                                       const int* __restrict__ stats, const int* __restrict__ table, int HW, CleanRule rule) {
  const int t = threadIdx.x, f = blockIdx.y;
  const unsigned char* s = src + (size_t)f * HW;
  unsigned char* d = dst + (size_t)f * HW;
  const int* R = roots + (size_t)f * HW;
  const int* S = stats + (size_t)f * HW * 4;
  const int* T = table + (size_t)f * 768;
  int head = (int)((16u - (unsigned)((uintptr_t)d & 15u)) & 15u);
  if (head > HW) head = HW;
  const int nchunks = (HW - head) >> 4;
  const int tail_begin = head + 16 * nchunks, tail = HW - tail_begin;
  const bool src_wide = (((uintptr_t)s + head) & 15u) == 0;        // uniform per frame
  const bool roots_wide = (((uintptr_t)(R + head)) & 15u) == 0;
  int last_r = -1, last_o = 0;
  for (int c = blockIdx.x * kThreads + t; c < nchunks; c += gridDim.x * kThreads) {
    const int p = head + 16 * c;
    uint4 w;
    if (src_wide) w = *(const uint4*)(s + p);
    else w = make_uint4(load4(s + p), load4(s + p + 4), load4(s + p + 8), load4(s + p + 12));
    int4 r[4];
    if (roots_wide) {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = *(const int4*)(R + p + 4 * k);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = make_int4(R[p + 4 * k], R[p + 4 * k + 1], R[p + 4 * k + 2], R[p + 4 * k + 3]);
    }
    uint4 o;
    o.x = clean4(w.x, r[0].x, r[0].y, r[0].z, r[0].w, last_r, last_o, S, T, HW, rule);
    o.y = clean4(w.y, r[1].x, r[1].y, r[1].z, r[1].w, last_r, last_o, S, T, HW, rule);
    o.z = clean4(w.z, r[2].x, r[2].y, r[2].z, r[2].w, last_r, last_o, S, T, HW, rule);
    o.w = clean4(w.w, r[3].x, r[3].y, r[3].z, r[3].w, last_r, last_o, S, T, HW, rule);
    *(uint4*)(d + p) = o;
  }
  if (blockIdx.x == 0) {
    int p = -1;
    if (t < head) p = t;
    else if (t >= 16 && t - 16 < tail) p = tail_begin + t - 16;
    if (p >= 0) d[p] = (unsigned char)clean_one(s[p], R[p], S, T, HW, rule);
  }
}

}  // namespace

extern "C" int rmem_label_components_tile(int* th, int* tw) {
  RMEM_REQUIRE(th && tw, "rmem_label_components_tile: null pointer (th and tw are required)");
  *th = kTH;
  *tw = kTW;
  return 0;
}

extern "C" long long rmem_label_components_workspace_bytes(int n, int H, int W) {
  if (!stack_geometry_ok(n, H, W)) return 0;
  return (long long)n * ((long long)H * W * 20 + 256 * 3 * 4);     // roots, stats (4 ints per pixel), table
}

extern "C" int rmem_label_components(const unsigned char* labels, int n, int H, int W, int connectivity, int* roots, int* status,
                                     void* stream) {
  RMEM_REQUIRE(labels && roots && status, "rmem_label_components: null pointer (labels, roots and status are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_components: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_components: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(connectivity == 4 || connectivity == 8, "rmem_label_components: connectivity must be 4 or 8");
  const int HW = H * W, conn8 = connectivity == 8;
  const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
  const dim3 tiles((unsigned)tiles_x * (unsigned)tiles_y, n);
  hipLaunchKernelGGL(k_cc_tile, tiles, dim3(kThreads), 0, (hipStream_t)stream, labels, (size_t)n * HW, H, W, tiles_x, conn8, roots, status);
  if (tiles.x > 1) hipLaunchKernelGGL(k_cc_seam, tiles, dim3(kSeamThreads), 0, (hipStream_t)stream, labels, H, W, tiles_x, conn8, roots, status);
  hipLaunchKernelGGL(k_cc_flatten, dim3((HW + kThreads - 1) / kThreads, n), dim3(kThreads), 0, (hipStream_t)stream, HW, roots, status);
  return rmem_check_launch("rmem_label_components");
}

extern "C" int rmem_label_component_stats(const unsigned char* labels, const int* roots, int n, int H, int W, int connectivity, int* stats,
                                          int* table, void* stream) {
  RMEM_REQUIRE(labels && roots && stats && table, "rmem_label_component_stats: null pointer (labels, roots, stats and table are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_component_stats: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_component_stats: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(connectivity == 4 || connectivity == 8, "rmem_label_component_stats: connectivity must be 4 or 8");
  const int HW = H * W, conn8 = connectivity == 8;
  const int init_threads = HW * 4 > 768 ? HW * 4 : 768;
  hipLaunchKernelGGL(k_cc_init, dim3((init_threads + kThreads - 1) / kThreads, n), dim3(kThreads), 0, (hipStream_t)stream, stats, HW * 4, table);
  hipLaunchKernelGGL(k_cc_stats, dim3((HW + 4 * kThreads - 1) / (4 * kThreads), n), dim3(kThreads), 0, (hipStream_t)stream, labels, roots, H, W,
                     conn8, stats);
  const dim3 grid(blocks_per_frame(16L * HW, n), n);              // one pixel per thread at the finest
  hipLaunchKernelGGL(k_cc_table_count, grid, dim3(kThreads), 0, (hipStream_t)stream, labels, roots, HW, stats, table);
  hipLaunchKernelGGL(k_cc_table_root, grid, dim3(kThreads), 0, (hipStream_t)stream, labels, roots, HW, stats, table);
  return rmem_check_launch("rmem_label_component_stats");
}

extern "C" int rmem_label_clean(const unsigned char* src, unsigned char* dst, const int* roots, const int* stats, const int* table, int n,
                                int H, int W, int max_hole_area, int max_sprinkle_area, int keep_largest, void* stream) {
  RMEM_REQUIRE(src && dst && roots && stats && table, "rmem_label_clean: null pointer (src, dst, roots, stats and table are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_clean: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_clean: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(max_hole_area >= 0 && max_sprinkle_area >= 0, "rmem_label_clean: max_hole_area and max_sprinkle_area must not be negative");
  const int HW = H * W;
  const CleanRule rule = {max_hole_area, max_sprinkle_area, keep_largest != 0};
  hipLaunchKernelGGL(k_cc_clean, dim3(blocks_per_frame(HW, n), n), dim3(kThreads), 0, (hipStream_t)stream, src, dst, roots, stats, table, HW,
                     rule);
  return rmem_check_launch("rmem_label_clean");
}
