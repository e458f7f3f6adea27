// Shape census of uint8 label stacks (include/rmem.h, rmem_label_moments / rmem_label_hull_count / rmem_label_hull_offsets /
// rmem_label_hull_write): the raw moments up to order two of every label value, the x extent of every object on every image row,
// and from those extents alone the convex hull of every object's pixel squares.  Integers only; element-type agnostic: built once.
//
//   k_shape_rows   A wave owns an image row and walks it 64 x 16 bytes at a time.  A row may start at any byte (W odd): the pieces
//                  are the 16-byte aligned ones that overlap it, a byte mask clips the first and the last, and a piece that is
//                  not wholly inside the stack is read byte by byte.  The distinct-value loop of k_census picks a value v; lanes
//                  are in x order, so the first and the last lane with a hit give xmin and xmax.  y is constant: with u the byte's
//                  position in the wave's step (0..1023, x = X0 + u) the wave needs a = sum 1, sum u and sum u^2 -- all below 2^31
//                  -- and one lane's worth of 64-bit arithmetic turns them into the six sums.  When the hits are one run (what a
//                  row of a blob is, and a uniform wave) the three are closed forms of the run's ends and nothing is reduced;
//                  otherwise every lane takes them from its 16-bit mask by population counts and the wave adds them up.  The
//                  workgroup's 6 x 256 table lives in LDS as 64-bit words, its non-empty entries are flushed with 64-bit global
//                  atomic adds (order-free, so bit-reproducible; the caller zeroes the table).  The row's extents are kept by the
//                  owning wave in LDS and written, absent ones included, when the row is done: no init pass, no atomics.
//   k_hull_flags   One wave per (frame, object).  Corner level l lies between rows l - 1 and l; its candidates are
//                  L[l] = min(xmin[l-1], xmin[l]) and R[l] = max(xmax[l-1], xmax[l]) + 1.  The left chain is the convex minorant
//                  of L over the levels, the right chain the concave majorant of R: one serial stack walk (monotone chain) per
//                  chain, O(h), the stack in LDS; turns are cross products below 2^29.  Two flag bits per level and the vertex
//                  count per object go out.  (The parallel O(h^2) membership form was measured and lost where it matters:
//                  experiments/hull_membership.diff.)
//   k_hull_write   After the exclusive scan of the counts (label_scan.h): scans the flags of an object and writes its ring, from
//                  (L, top) east to (R, top), down the right chain, west along the bottom and up the left chain.
#include <limits.h>
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
constexpr int kMaxSide = 16384;       // the sums stay below 2^55, the slope products below 2^29

__device__ __forceinline__ int top_bit(unsigned m) { return 31 - __builtin_clz(m); }
// sum of the bit positions j of m (16 bits), and of their squares: j = sum_b 2^b j_b
__device__ __forceinline__ int sum_j(unsigned m) {
  return __popc(m & 0xaaaau) + 2 * __popc(m & 0xccccu) + 4 * __popc(m & 0xf0f0u) + 8 * __popc(m & 0xff00u);
}
__device__ __forceinline__ int sum_jj(unsigned m) {
  return __popc(m & 0xaaaau) + 4 * __popc(m & 0xccccu) + 16 * __popc(m & 0xf0f0u) + 64 * __popc(m & 0xff00u) +
         4 * __popc(m & 0x8888u) + 8 * __popc(m & 0xa0a0u) + 16 * __popc(m & 0xaa00u) + 16 * __popc(m & 0xc0c0u) +
         32 * __popc(m & 0xcc00u) + 64 * __popc(m & 0xf000u);
}
// 0^2 + 1^2 + ... + k^2, k in -1..1023
__device__ __forceinline__ long long squares_to(int k) { return (long long)k * (k + 1) * (2 * k + 1) / 6; }

// One wave's step: lane l holds the bytes `rem` (a 16-bit mask; 0 = nothing) of w; byte j of lane l is the pixel (X0 + 16 l + j, y).
// tab: the workgroup's moments; ext: the wave's extents of this row (value -> xmin, xmax).  Called by whole waves only.
template <bool MOM, bool EXT>
__device__ __forceinline__ void wave_shapes(uint4 w, unsigned rem, int y, int X0, int num, int lane, unsigned long long (*tab)[256],
                                            int (*ext)[2]) {
  const bool uni = rem == 0xffffu && all_equal(w);
  const int first = (int)(w.x & 0xffu);
  for (;;) {
    const uint64_t busy = __ballot(rem != 0);
    if (!busy) break;
    const int cand = byte_at(w, rem ? __builtin_ctz(rem) : 0);
    const int v = __builtin_amdgcn_readlane(cand, __builtin_ctzll(busy));
    const unsigned m = uni ? (first == v ? 0xffffu : 0u) : (eq16(w, v) & rem);
    rem &= ~m;
    const uint64_t hit = __ballot(m != 0);         // never empty: the lane v was picked from holds it
    const int lo = __builtin_ctzll(hit), hi = 63 - __builtin_clzll(hit);
    const unsigned mlo = (unsigned)__builtin_amdgcn_readlane((int)m, lo), mhi = (unsigned)__builtin_amdgcn_readlane((int)m, hi);
    const int zlo = __builtin_ctz(mlo);
    const int u0 = 16 * lo + zlo, u1 = 16 * hi + top_bit(mhi);
    if (EXT && v >= 1 && v <= num && lane == 0) {
      ext[v][0] = min(ext[v][0], X0 + u0);
      ext[v][1] = max(ext[v][1], X0 + u1);
    }
    if (!MOM) continue;
    bool run;                                      // the hits are the bytes u0..u1 and nothing else
    if (lo == hi) {
      const unsigned t = mlo >> zlo;
      run = (t & (t + 1u)) == 0u;
    } else {
      const uint64_t between = hi > lo + 1 ? ((~0ull >> (64 - hi)) & (~0ull << (lo + 1))) : 0ull;     // lanes lo + 1 .. hi - 1
      run = (__ballot(m == 0xffffu) & between) == between && (mlo >> zlo) == (0xffffu >> zlo) && (mhi & (mhi + 1u)) == 0u;
    }
    long long a, su, suu;
    if (run) {
      a = u1 - u0 + 1;
      su = (long long)(u0 + u1) * a / 2;
      suu = squares_to(u1) - squares_to(u0 - 1);
    } else {
      const int pa = __popc(m), ul = 16 * lane, pj = pa * ul + sum_j(m);
      a = wave_isum(pa);
      su = wave_isum(pj);
      suu = wave_isum(pa * ul * ul + 2 * ul * sum_j(m) + sum_jj(m));     // at most 0^2 + ... + 1023^2 < 2^29
    }
    const long long sx = a * X0 + su, sxx = a * X0 * X0 + 2ll * X0 * su + suu;
    const long long val = lane == 0 ? a : lane == 1 ? sx : lane == 2 ? a * y : lane == 3 ? sxx : lane == 4 ? sx * y : a * y * y;
    if (lane < 6) atomicAdd(&tab[lane][v], (unsigned long long)val);
  }
}

template <bool MOM, bool EXT>
__global__ __launch_bounds__(kThreads) void k_shape_rows(const unsigned char* __restrict__ labels, int n, int H, int W, int num,
                                                         unsigned long long* __restrict__ mom, int* __restrict__ extents) {
  __shared__ unsigned long long tab[MOM ? 6 : 1][256];
  __shared__ int rowext[EXT ? kWaves : 1][256][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, f = blockIdx.y;
  if (MOM) {
#pragma unroll
    for (int k = 0; k < 6; ++k) tab[k][t] = 0;
  }
  int (*ext)[2] = rowext[EXT ? wave : 0];
  if (EXT) {
    for (int v = lane; v < 256; v += 64) { ext[v][0] = W; ext[v][1] = -1; }
  }
  __syncthreads();
  const size_t HW = (size_t)H * W;
  const uintptr_t stack_begin = (uintptr_t)labels, stack_end = stack_begin + (size_t)n * HW;
  const unsigned char* base = labels + (size_t)f * HW;
  for (int y = blockIdx.x * kWaves + wave; y < H; y += gridDim.x * kWaves) {
    const unsigned char* row = base + (size_t)y * W;
    const int lead = (int)((uintptr_t)row & 15u);                  // bytes of the first aligned piece that precede the row
    const unsigned char* arow = row - lead;
    const int pieces = (lead + W + 15) >> 4;
    for (int p0 = 0; p0 < pieces; p0 += 64) {
      const int p = p0 + lane;
      uint4 w = make_uint4(0, 0, 0, 0);
      unsigned rem = 0;
      if (p < pieces) {
        const int xl = 16 * p - lead;                              // x of the piece's byte 0: -15 .. W - 1
        rem = 0xffffu;
        if (xl < 0) rem &= 0xffffu << -xl;
        if (xl + 16 > W) rem &= 0xffffu >> (xl + 16 - W);
        const unsigned char* a = arow + 16 * (size_t)p;
        if ((uintptr_t)a >= stack_begin && (uintptr_t)a + 16 <= stack_end) {
          w = *(const uint4*)a;
        } else {                                                   // the stack's first and last piece: its own bytes only
          uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if ((rem >> j) & 1u) q[j >> 2] |= (uint32_t)a[j] << (8 * (j & 3));
          w = make_uint4(q[0], q[1], q[2], q[3]);
        }
      }
      wave_shapes<MOM, EXT>(w, rem, y, 16 * p0 - lead, num, lane, tab, ext);
    }
    if (EXT) {
      __builtin_amdgcn_wave_barrier();
      for (int v = 1 + lane; v <= num; v += 64) {
        int* o = extents + (((size_t)f * num + (v - 1)) * H + y) * 2;
        o[0] = ext[v][0]; o[1] = ext[v][1];
        ext[v][0] = W; ext[v][1] = -1;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (MOM) {
    __syncthreads();
    if (tab[0][t]) {
      unsigned long long* o = mom + ((size_t)f * 256 + t) * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) atomicAdd(o + k, tab[k][t]);
    }
  }
}

// the candidates of corner level l (0..H) from an object's row extents e [H][2]; W and 0 say "none" (both or neither)
__device__ __forceinline__ int level_L(const int* __restrict__ e, int l, int H, int W) {
  return min(l > 0 ? e[2 * (l - 1)] : W, l < H ? e[2 * l] : W);
}
__device__ __forceinline__ int level_R(const int* __restrict__ e, int l, int H) {
  return max(l > 0 ? e[2 * (l - 1) + 1] : -1, l < H ? e[2 * l + 1] : -1) + 1;
}

// One wave per (frame, object).  Both chains are walked with the monotone-chain stack, entry = level << 16 | value; the bottom
// entry is never popped and stays in registers, so H entries (4 H bytes of dynamic LDS) hold the H + 1 levels.  The wave loads 64
// levels at a time; the walk is uniform, lane 0 writes the stack.
__global__ __launch_bounds__(64) void k_hull_flags(const int* __restrict__ extents, int H, int W, unsigned char* __restrict__ flags,
                                                   int* __restrict__ counts) {
  extern __shared__ unsigned st[];
  const int lane = threadIdx.x;
  const size_t obj = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int* e = extents + obj * H * 2;
  unsigned char* fl = flags + obj * (H + 1);
  int y0 = INT_MAX, y1 = -1;
  for (int y = lane; y < H; y += 64)
    if (e[2 * y + 1] >= 0) { y0 = min(y0, y); y1 = y; }
  y0 = wave_imin(y0); y1 = wave_imax(y1);
  for (int i = lane; i <= H; i += 64) fl[i] = 0;
  if (y1 < 0) {
    if (lane == 0) counts[obj] = 0;
    return;
  }
  __syncthreads();
  const int l0 = y0, l1 = y1 + 1;
  int total = 0;
  for (int chain = 0; chain < 2; ++chain) {
    const int sign = chain ? -1 : 1;
    const int bl = l0, bv = chain ? level_R(e, l0, H) : level_L(e, l0, H, W);
    int sp = 0, tl = bl, tv = bv, ul = bl, uv = bv;                // entries above the bottom; the top entry and the one under it
    for (int c = l0 + 1; c <= l1; c += 64) {
      const int l = c + lane;
      const int val = l <= l1 ? (chain ? level_R(e, l, H) : level_L(e, l, H, W)) : (chain ? 0 : W);
      const int m = min(64, l1 - c + 1);
      for (int q = 0; q < m; ++q) {
        const int v = __builtin_amdgcn_readlane(val, q), lev = c + q;
        if (chain ? v == 0 : v >= W) continue;
        while (sp >= 1 && sign * ((tl - ul) * (v - tv) - (tv - uv) * (lev - tl)) <= 0) {
          --sp;
          tl = ul; tv = uv;
          if (sp >= 2) { const unsigned u = st[sp - 2]; ul = (int)(u >> 16); uv = (int)(u & 0xffffu); }
          else { ul = bl; uv = bv; }
        }
        if (lane == 0) st[sp] = ((unsigned)lev << 16) | (unsigned)v;
        ++sp;
        ul = tl; uv = tv; tl = lev; tv = v;
      }
    }
    __syncthreads();
    for (int k = lane; k <= sp; k += 64) {
      const int lev = k == 0 ? l0 : (int)(st[k - 1] >> 16);
      fl[lev] |= (unsigned char)(1 << chain);
    }
    total += sp + 1;
    __syncthreads();
  }
  if (lane == 0) counts[obj] = total;
}

__global__ __launch_bounds__(kThreads) void k_hull_write(const int* __restrict__ extents, const unsigned char* __restrict__ flags, int H, int W,
                                                         const int* __restrict__ offsets, int* __restrict__ verts, int capacity) {
  __shared__ int sh[kWaves];
  const int t = threadIdx.x;
  const size_t obj = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int off = offsets[obj], total = offsets[obj + 1] - off;
  if (total <= 0 || off < 0 || off + total > capacity) return;     // uniform; the last two never hold for the scan of these flags' counts
  const int* e = extents + obj * H * 2;
  const unsigned char* fl = flags + obj * (H + 1);
  int carry = 0;                                                   // vertices on earlier levels: right chain | left chain << 16
  for (int ib = 0; ib <= H; ib += kThreads) {
    const int i = ib + t;
    const int bits = i <= H ? fl[i] : 0;
    const int v = (bits >> 1) | ((bits & 1) << 16);
    int tot;
    const int before = carry + block_incl_scan(v, sh, tot) - v;
    carry += tot;
    if (bits & 2) {
      const int pos = 1 + (before & 0xffff);
      if (pos < total) { verts[2 * (size_t)(off + pos)] = level_R(e, i, H); verts[2 * (size_t)(off + pos) + 1] = i; }
    }
    if (bits & 1) {
      int pos = total - (before >> 16);
      if (pos == total) pos = 0;
      if (pos >= 0) { verts[2 * (size_t)(off + pos)] = level_L(e, i, H, W); verts[2 * (size_t)(off + pos) + 1] = i; }
    }
  }
}

inline bool shapes_geometry_ok(int n, int H, int W) { return stack_geometry_ok(n, H, W) && H <= kMaxSide && W <= kMaxSide; }
}  // namespace

extern "C" int rmem_label_moments(const unsigned char* labels, int n, int H, int W, int num, long long* moments, int* extents, void* stream) {
  RMEM_REQUIRE(labels && (moments || extents), "rmem_label_moments: null pointer (labels and one of moments, extents are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_moments: n must be in 1..65535");
  RMEM_REQUIRE(shapes_geometry_ok(n, H, W), "rmem_label_moments: H and W must be in 1..16384, H * W at most 2^26");
  RMEM_REQUIRE(!extents || (num >= 1 && num <= 255), "rmem_label_moments: num must be in 1..255");
  hipStream_t s = (hipStream_t)stream;
  if (moments && hipMemsetAsync(moments, 0, (size_t)n * 256 * 6 * sizeof(long long), s) != hipSuccess) {
    rmem_set_error("rmem_label_moments: hipMemsetAsync failed");
    return -1;
  }
  const int cap = kMaxBlocks / n > 1 ? kMaxBlocks / n : 1;
  int bx = (H + kWaves - 1) / kWaves;
  if (bx > cap) bx = cap;
  const dim3 grid(bx, n), block(kThreads);
  unsigned long long* mom = (unsigned long long*)moments;
  if (moments && extents) hipLaunchKernelGGL((k_shape_rows<true, true>), grid, block, 0, s, labels, n, H, W, num, mom, extents);
  else if (moments) hipLaunchKernelGGL((k_shape_rows<true, false>), grid, block, 0, s, labels, n, H, W, 0, mom, extents);
  else hipLaunchKernelGGL((k_shape_rows<false, true>), grid, block, 0, s, labels, n, H, W, num, mom, extents);
  return rmem_check_launch("rmem_label_moments");
}

extern "C" int rmem_label_hull_count(const int* extents, int n, int H, int W, int num, unsigned char* flags, int* counts, void* stream) {
  RMEM_REQUIRE(extents && flags && counts, "rmem_label_hull_count: null pointer (extents, flags and counts are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_hull_count: n must be in 1..65535");
  RMEM_REQUIRE(shapes_geometry_ok(n, H, W), "rmem_label_hull_count: H and W must be in 1..16384, H * W at most 2^26");
  RMEM_REQUIRE(num >= 1 && num <= 255, "rmem_label_hull_count: num must be in 1..255");
  hipLaunchKernelGGL(k_hull_flags, dim3(num, n), dim3(64), (size_t)H * sizeof(unsigned), (hipStream_t)stream, extents, H, W, flags, counts);
  return rmem_check_launch("rmem_label_hull_count");
}

extern "C" int rmem_label_hull_offsets(int* counts, int objects, void* stream) {
  RMEM_REQUIRE(counts, "rmem_label_hull_offsets: null pointer (counts is required)");
  RMEM_REQUIRE(objects >= 1 && objects <= kMaxFrames * 255, "rmem_label_hull_offsets: objects must be in 1..65535 * 255");
  hipLaunchKernelGGL(k_label_scan_units, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, counts, objects, counts + objects);
  return rmem_check_launch("rmem_label_hull_offsets");
}

extern "C" int rmem_label_hull_write(const int* extents, const unsigned char* flags, int n, int H, int W, int num, const int* offsets,
                                     int* verts, long long capacity, void* stream) {
  RMEM_REQUIRE(extents && flags && offsets && verts, "rmem_label_hull_write: null pointer (extents, flags, offsets and verts are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_hull_write: n must be in 1..65535");
  RMEM_REQUIRE(shapes_geometry_ok(n, H, W), "rmem_label_hull_write: H and W must be in 1..16384, H * W at most 2^26");
  RMEM_REQUIRE(num >= 1 && num <= 255, "rmem_label_hull_write: num must be in 1..255");
  RMEM_REQUIRE(capacity >= 1 && capacity <= INT_MAX, "rmem_label_hull_write: capacity must be in 1..2^31-1");
  hipLaunchKernelGGL(k_hull_write, dim3(num, n), dim3(kThreads), 0, (hipStream_t)stream, extents, flags, H, W, offsets, verts, (int)capacity);
  return rmem_check_launch("rmem_label_hull_write");
}
