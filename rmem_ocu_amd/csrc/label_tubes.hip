// Label pieces through time (include/rmem.h: rmem_label_tubes, rmem_label_tube_lineage, rmem_label_tube_events, rmem_label_tube_index,
// rmem_label_tube_table, rmem_label_tube_clean): the pieces of rmem_label_components joined over consecutive frames into tubes, the
// lineage of every piece, the per-frame events, the table of tubes and the clean-up rule in time (tubes.py).  Element-type agnostic
// (uint8 / int32 in, int32 / uint8 out): built once.
//
// A voxel's global index is g = f * H * W + y * W + x (n * H * W <= 2^31 - 1: it fits an int).  The same union-find as
// label_components.hip, over global indices: the smaller index always wins, so a tube's representative is its first voxel in
// frame-major raster order whatever the schedule.  Separate launches; no kernel waits for or spins on another workgroup; every loop
// that walks parents carries a bound, and reaching one sets a bit of the caller's status word (bit 0: union, bit 1: find).
//
//   k_tube_parents  tubes[g] = f * HW + roots[f][p]: the parent forest starts as the 2-D pieces.
//   k_tube_link     One lane per pixel of frame f >= 1.  Per temporal offset (1 or 9) the lane's pair (its piece, the piece of the
//                   pixel of the same value on frame f - 1).  A lane drops a pair equal to its left neighbour's (and, under 9, to
//                   its own pair at the previous offset); then the wave picks, from the first lane that has a pair left, one leader
//                   per distinct pair (ballot + readlane, at most 64 rounds), and only leaders act: for the tubes a union (finds
//                   with relaxed agent-scope loads, atomicMin(&parent[larger], smaller), only the returned value decides, no
//                   atomic when the two finds meet), for the lineage the four extrema -- an integer min / max each, not sent
//                   where a relaxed load shows that it would change nothing (the words only move one way).
//   k_tube_flatten  tubes[g] = find(g), in place.
//   k_tube_fill4    the (H * W, -1, H * W, -1) of the lineage and the zeros of the events.
//   k_tube_events   Per frame the roots' (born, ended, splitting, merging) into an LDS table [256][4] per workgroup, flushed with adds.
//   k_tube_count, k_tube_scan, k_tube_rank
//                   count-then-write with label_scan.h: a workgroup counts the tube ids (tubes[g] == g) of its chunk into the
//                   chunk's first entry of rank, one workgroup scans those entries, the chunks write rank from their offset.
//   k_tube_rows, k_tube_table
//                   Row rank[g] = (g, value, 0, 0, f, f, 256, -1, 0, 0) at every tube id; then every piece root adds its area, 1,
//                   its frame, its neighbour extrema, its border bit and its area as a maximum to its tube's row.
//   k_tube_clean    dst from src, roots, stats, tubes, rank and table over the flat stack; 16 voxels per lane, 16-byte stores where
//                   dst allows, single bytes at head and tail; every byte is read and written by the same thread, and read first
//                   (dst == src is allowed).  A lane keeps the last piece's decision.
#include <limits.h>
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
constexpr int kStatusUnion = 1, kStatusFind = 2;
constexpr int kRankPerThread = 16;                // voxels per thread of the count / rank passes, at least
constexpr int kRankBlocks = 16384;                // chunks of those passes, at most: what one workgroup scans
constexpr int kCols = 10;                         // columns of a table row

// ------------------------------------------------------------------------------------------------------------- the forest
__device__ __forceinline__ int t_find(int* par, int x, int N, int* status) {
  for (unsigned it = 0; it <= (unsigned)N; ++it) {
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    if ((unsigned)p >= (unsigned)N) break;         // never: not a parent k_tube_parents wrote
    x = p;
  }
  atomicOr(status, kStatusFind);
  return -1;
}
__device__ __forceinline__ void t_union(int* par, int a, int b, int N, int* status) {
  a = t_find(par, a, N, status);
  b = t_find(par, b, N, status);
  if (a < 0 || b < 0) return;
  for (unsigned it = 0; it < (unsigned)N + 64u; ++it) {
    if (a == b) return;                            // the finds meet: no atomic
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;                          // a was a root and hangs below b now
    a = old;                                       // a had a parent: that one and b remain to be united
  }
  atomicOr(status, kStatusUnion);
}

__global__ __launch_bounds__(kThreads) void k_tube_parents(const int* __restrict__ roots, int HW, int* __restrict__ tubes) {
  const int p = blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y;
  if (p >= HW) return;
  const size_t g = (size_t)f * HW + p;
  const int r = roots[g];
  tubes[g] = (unsigned)r < (unsigned)HW ? f * HW + r : (int)g;     // anything else is not a root of rmem_label_components: a piece of its own
}

// whole waves only: true in exactly one lane per distinct (a, b) among the lanes with has
__device__ __forceinline__ bool wave_pair_leader(bool has, int a, int b, int lane) {
  const int la = __shfl_up(a, 1, 64), lb = __shfl_up(b, 1, 64), lh = __shfl_up((int)has, 1, 64);
  if (lane > 0 && lh && la == a && lb == b) has = false;           // the left neighbour holds the same pair
  bool lead = false;
  for (int round = 0; round < 64; ++round) {                       // every round settles its first lane at least
    const uint64_t busy = __ballot(has);
    if (!busy) break;
    const int first = __builtin_ctzll(busy);
    const int a0 = __builtin_amdgcn_readlane(a, first), b0 = __builtin_amdgcn_readlane(b, first);
    if (has && a == a0 && b == b0) {
      has = false;
      lead = lane == first;
    }
  }
  return lead;
}

__device__ __forceinline__ void link_min(int* w, int v) {
  if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(w, v);
}
__device__ __forceinline__ void link_max(int* w, int v) {
  if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(w, v);
}

// kLineage = false: unions in the forest `out` (tubes); true: the extrema in `out` (links).  Frame f = blockIdx.y + 1 against f - 1.
template <bool kLineage>
__global__ __launch_bounds__(kThreads) void k_tube_link(const unsigned char* __restrict__ labels, const int* __restrict__ roots, int H, int W,
                                                        int N, int wide, int* out, int* __restrict__ status) {
  const int lane = threadIdx.x & 63, f = blockIdx.y + 1;
  const int HW = H * W;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  const bool live = p < HW;
  const unsigned char* L1 = labels + (size_t)f * HW;
  const unsigned char* L0 = L1 - HW;
  const int* R1 = roots + (size_t)f * HW;
  const int* R0 = R1 - HW;
  int me = -1, a = 0, y = 0, x = 0;
  bool mine = false;
  if (live) {
    me = L1[p];
    a = R1[p];
    mine = (unsigned)a < (unsigned)HW;
    y = p / W;
    x = p - y * W;
  }
  int last_b = -1;
  const int reach = wide ? 1 : 0;
  for (int dy = -reach; dy <= reach; ++dy) {
    for (int dx = -reach; dx <= reach; ++dx) {
      bool has = false;
      int b = 0;
      if (mine && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W) {
        const int q = p + dy * W + dx;
        if (L0[q] == me) {
          b = R0[q];
          has = (unsigned)b < (unsigned)HW && b != last_b;         // the pair of the previous offset is made already
          if (has) last_b = b;
        }
      }
      if (!wave_pair_leader(has, a, b, lane)) continue;
      if (kLineage) {
        int* mine4 = out + ((size_t)f * HW + a) * 4;
        int* theirs4 = out + ((size_t)(f - 1) * HW + b) * 4;
        link_min(mine4 + 0, b);
        link_max(mine4 + 1, b);
        link_min(theirs4 + 2, a);
        link_max(theirs4 + 3, a);
      } else {
        t_union(out, f * HW + a, (f - 1) * HW + b, N, status);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_tube_flatten(int N, int* tubes, int* __restrict__ status) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= (size_t)N) return;
  const int r = t_find(tubes, (int)g, N, status);
  if (r >= 0) tubes[g] = r;
}

// ------------------------------------------------------------------------------------------------------ lineage and events
__global__ __launch_bounds__(kThreads) void k_tube_fill4(int4* __restrict__ out, size_t count, int4 v) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (size_t)gridDim.x * kThreads) {
    int* o = (int*)(out + i);                      // four words: the caller's buffer need not be 16-byte aligned
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
}

__global__ __launch_bounds__(kThreads) void k_tube_events(const unsigned char* __restrict__ labels, const int* __restrict__ roots,
                                                          const int* __restrict__ links, int n, int HW, int* __restrict__ events) {
  __shared__ int cnt[256 * 4];
  const int t = threadIdx.x, f = blockIdx.y;
#pragma unroll
  for (int k = 0; k < 4; ++k) cnt[k * kThreads + t] = 0;
  __syncthreads();
  const unsigned char* L = labels + (size_t)f * HW;
  const int* R = roots + (size_t)f * HW;
  const int* K = links + (size_t)f * HW * 4;
  for (int p = blockIdx.x * kThreads + t; p < HW; p += gridDim.x * kThreads) {
    if (R[p] != p) continue;
    const int v = L[p];
    const int* k4 = K + (size_t)p * 4;
    const int prev_min = k4[0], prev_max = k4[1], next_min = k4[2], next_max = k4[3];
    if (f >= 1 && prev_max < 0) atomicAdd(&cnt[v * 4 + 0], 1);
    if (f <= n - 2 && next_max < 0) atomicAdd(&cnt[v * 4 + 1], 1);
    if (next_max >= 0 && next_min != next_max) atomicAdd(&cnt[v * 4 + 2], 1);
    if (prev_max >= 0 && prev_min != prev_max) atomicAdd(&cnt[v * 4 + 3], 1);
  }
  __syncthreads();
  int* E = events + (size_t)f * 1024;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cnt[k * kThreads + t];
    if (c) atomicAdd(E + k * kThreads + t, c);
  }
}

// ------------------------------------------------------------------------------------------------------------------ index
// chunk b = voxels [b * per, (b + 1) * per), per = kThreads * per_thread; thread t takes b * per + j * kThreads + t
__global__ __launch_bounds__(kThreads) void k_tube_count(const int* __restrict__ tubes, int N, int per_thread, int* __restrict__ rank) {
  __shared__ int sh[kWaves];
  const size_t base = (size_t)blockIdx.x * kThreads * per_thread;
  int c = 0;
  for (int j = 0; j < per_thread; ++j) {
    const size_t g = base + (size_t)j * kThreads + threadIdx.x;
    if (g < (size_t)N && tubes[g] == (int)g) ++c;
  }
  c = wave_isum(c);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += sh[k];
    rank[base] = s;
  }
}

// one workgroup: the chunks' counts (every `stride` entries of rank) to their exclusive scan in place, the sum to total
__global__ __launch_bounds__(kThreads) void k_tube_scan(int* __restrict__ rank, int chunks, size_t stride, int* __restrict__ total) {
  __shared__ int sh[kWaves];
  int carry = 0;
  for (int b = 0; b < chunks; b += kThreads) {
    const int i = b + threadIdx.x;
    const int v = i < chunks ? rank[(size_t)i * stride] : 0;
    int tot;
    const int inc = block_incl_scan(v, sh, tot);
    if (i < chunks) rank[(size_t)i * stride] = carry + inc - v;
    carry += tot;
  }
  if (threadIdx.x == 0) total[0] = carry;
}

__global__ __launch_bounds__(kThreads) void k_tube_rank(const int* __restrict__ tubes, int N, int per_thread, int* rank) {
  __shared__ int sh[kWaves];
  const size_t base = (size_t)blockIdx.x * kThreads * per_thread;
  int carry = rank[base];                          // the chunk's offset: read by every thread before thread 0 overwrites it
  __syncthreads();
  for (int j = 0; j < per_thread; ++j) {
    const size_t g = base + (size_t)j * kThreads + threadIdx.x;
    const int is = g < (size_t)N && tubes[g] == (int)g ? 1 : 0;
    int tot;
    const int inc = block_incl_scan(is, sh, tot);
    if (g < (size_t)N) rank[g] = is ? carry + inc - 1 : -1;
    carry += tot;
  }
}

// ------------------------------------------------------------------------------------------------------------------ table
__global__ __launch_bounds__(kThreads) void k_tube_rows(const unsigned char* __restrict__ labels, const int* __restrict__ tubes,
                                                        const int* __restrict__ rank, int N, int HW, int rows, int* __restrict__ table) {
  for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < (size_t)N; g += (size_t)gridDim.x * kThreads) {
    if (tubes[g] != (int)g) continue;
    const int k = rank[g];
    if ((unsigned)k >= (unsigned)rows) continue;
    const int f = (int)(g / (size_t)HW);
    int* o = table + (size_t)k * kCols;
    o[0] = (int)g; o[1] = labels[g]; o[2] = 0; o[3] = 0; o[4] = f; o[5] = f; o[6] = 256; o[7] = -1; o[8] = 0; o[9] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_tube_table(const int* __restrict__ roots, const int* __restrict__ stats,
                                                         const int* __restrict__ tubes, const int* __restrict__ rank, int N, int HW, int rows,
                                                         int* table) {
  for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < (size_t)N; g += (size_t)gridDim.x * kThreads) {
    const int f = (int)(g / (size_t)HW);
    if (roots[g] != (int)(g - (size_t)f * HW)) continue;            // piece roots only
    const int id = tubes[g];
    if ((unsigned)id >= (unsigned)N) continue;
    const int k = rank[id];
    if ((unsigned)k >= (unsigned)rows) continue;
    const int* s = stats + g * 4;
    const int area = s[0], lo = s[1], hi = s[2], border = s[3];
    int* o = table + (size_t)k * kCols;
    atomicAdd(o + 2, area);
    atomicAdd(o + 3, 1);
    link_max(o + 5, f);
    if (hi >= 0) {
      link_min(o + 6, lo);
      link_max(o + 7, hi);
    }
    if (border) link_max(o + 8, 1);
    link_max(o + 9, area);
  }
}

// ------------------------------------------------------------------------------------------------------------------ apply
struct TubeRule {
  int min_frames, max_hole_frames, n;
};

__device__ __forceinline__ int tube_clean_one(int v, int f, int r, const int* __restrict__ stats, const int* __restrict__ tubes,
                                              const int* __restrict__ rank, const int* __restrict__ table, int HW, int N, TubeRule rule) {
  if ((unsigned)r >= (unsigned)HW) return v;       // not a root of rmem_label_components: the voxel stays
  const size_t piece = (size_t)f * HW + r;
  const int id = tubes[piece];
  if ((unsigned)id >= (unsigned)N) return v;
  const int k = rank[id];
  if (k < 0) return v;
  const int* row = table + (size_t)k * kCols;
  const int f_first = row[4], f_last = row[5];
  if (f_first < 1 || f_last > rule.n - 2) return v;                // not closed: frame 0 is given, the last frame's tubes go on
  const int life = f_last - f_first + 1;
  if (v == 0) return life <= rule.max_hole_frames && row[8] == 0 && row[6] == row[7] ? row[6] : 0;
  if (life < rule.min_frames) {
    const int* s = stats + piece * 4;
    return s[1] == s[2] ? s[1] : 0;
  }
  return v;
}

// src and dst may be the same stack: every byte is read and written by the same thread, and read first.
__global__ __launch_bounds__(kThreads) void k_tube_clean(const unsigned char* src, unsigned char* dst, const int* __restrict__ roots,
                                                         const int* __restrict__ stats, const int* __restrict__ tubes,
                                                         const int* __restrict__ rank, const int* __restrict__ table, int HW, int N,
                                                         TubeRule rule) {
  const int t = threadIdx.x;
  int head = (int)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u);
  if (head > N) head = N;
  const int nchunks = (N - head) >> 4;
  const int tail_begin = head + 16 * nchunks, tail = N - tail_begin;
  const bool src_wide = (((uintptr_t)src + head) & 15u) == 0;
  const bool roots_wide = (((uintptr_t)(roots + head)) & 15u) == 0;
  int last_r = -1, last_f = -1, last_o = 0;
  for (size_t c = (size_t)blockIdx.x * kThreads + t; c < (size_t)nchunks; c += (size_t)gridDim.x * kThreads) {
    const size_t g0 = (size_t)head + 16 * c;
    int f = (int)(g0 / (size_t)HW);
    size_t next = (size_t)(f + 1) * HW;            // the first voxel of frame f + 1
    uint4 w;
    if (src_wide) w = *(const uint4*)(src + g0);
    else w = make_uint4(load4(src + g0), load4(src + g0 + 4), load4(src + g0 + 8), load4(src + g0 + 12));
    const uint32_t in[4] = {w.x, w.y, w.z, w.w};
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int4 r4;
      if (roots_wide) r4 = *(const int4*)(roots + g0 + 4 * q);
      else r4 = make_int4(roots[g0 + 4 * q], roots[g0 + 4 * q + 1], roots[g0 + 4 * q + 2], roots[g0 + 4 * q + 3]);
      const int rs[4] = {r4.x, r4.y, r4.z, r4.w};
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t g = g0 + 4 * q + j;
        if (g >= next) {                           // a frame of fewer than 16 pixels ends inside the chunk, several may
          f = (int)(g / (size_t)HW);
          next = (size_t)(f + 1) * HW;
        }
        const int v = (int)((in[q] >> (8 * j)) & 0xffu);
        if (rs[j] != last_r || f != last_f) {      // a piece holds one value: (frame, root) decides
          last_r = rs[j];
          last_f = f;
          last_o = tube_clean_one(v, f, rs[j], stats, tubes, rank, table, HW, N, rule);
        }
        word |= (uint32_t)last_o << (8 * j);
      }
      o[q] = word;
    }
    *(uint4*)(dst + g0) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  if (blockIdx.x == 0) {
    int g = -1;
    if (t < head) g = t;
    else if (t >= 16 && t - 16 < tail) g = tail_begin + t - 16;
    if (g >= 0) {
      const int f = g / HW;
      dst[g] = (unsigned char)tube_clean_one(src[g], f, roots[g], stats, tubes, rank, table, HW, N, rule);
    }
  }
}

// host: the stack as the entry points take it, whole
inline bool tube_geometry_ok(int n, int H, int W) { return stack_geometry_ok(n, H, W) && (long long)n * H * W <= (long long)INT_MAX; }
inline int flat_blocks(long long items) {
  long long b = (items + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)(b < 1 ? 1 : b);
}
}  // namespace

#define RMEM_TUBE_GEOMETRY(name)                                                                                    \
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, name ": n must be in 1..65535");                                           \
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), name ": H and W must be positive, H * W at most 2^26");                   \
  RMEM_REQUIRE(tube_geometry_ok(n, H, W), name ": n * H * W must be at most 2^31 - 1 (the stack is taken whole)")
#define RMEM_TUBE_TEMPORAL(name) RMEM_REQUIRE(temporal == 1 || temporal == 9, name ": temporal must be 1 or 9")

extern "C" long long rmem_label_tubes_workspace_bytes(int n, int H, int W) {
  if (!tube_geometry_ok(n, H, W)) return 0;
  return (long long)n * H * W * 28;                                // roots, stats (4 ints per voxel), tubes, rank
}

extern "C" int rmem_label_tubes(const unsigned char* labels, const int* roots, int n, int H, int W, int temporal, int* tubes, int* status,
                                void* stream) {
  RMEM_REQUIRE(labels && roots && tubes && status, "rmem_label_tubes: null pointer (labels, roots, tubes and status are required)");
  RMEM_TUBE_GEOMETRY("rmem_label_tubes");
  RMEM_TUBE_TEMPORAL("rmem_label_tubes");
  const int HW = H * W, N = n * HW;
  const dim3 frame((HW + kThreads - 1) / kThreads, n);
  hipLaunchKernelGGL(k_tube_parents, frame, dim3(kThreads), 0, (hipStream_t)stream, roots, HW, tubes);
  if (n > 1) {
    hipLaunchKernelGGL(k_tube_link<false>, dim3(frame.x, n - 1), dim3(kThreads), 0, (hipStream_t)stream, labels, roots, H, W, N, temporal == 9,
                       tubes, status);
    hipLaunchKernelGGL(k_tube_flatten, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, N, tubes, status);
  }
  return rmem_check_launch("rmem_label_tubes");
}

extern "C" int rmem_label_tube_lineage(const unsigned char* labels, const int* roots, int n, int H, int W, int temporal, int* links,
                                       void* stream) {
  RMEM_REQUIRE(labels && roots && links, "rmem_label_tube_lineage: null pointer (labels, roots and links are required)");
  RMEM_TUBE_GEOMETRY("rmem_label_tube_lineage");
  RMEM_TUBE_TEMPORAL("rmem_label_tube_lineage");
  const int HW = H * W, N = n * HW;
  hipLaunchKernelGGL(k_tube_fill4, dim3(flat_blocks(N)), dim3(kThreads), 0, (hipStream_t)stream, (int4*)links, (size_t)N, make_int4(HW, -1, HW, -1));
  if (n > 1)
    hipLaunchKernelGGL(k_tube_link<true>, dim3((HW + kThreads - 1) / kThreads, n - 1), dim3(kThreads), 0, (hipStream_t)stream, labels, roots, H, W,
                       N, temporal == 9, links, (int*)nullptr);
  return rmem_check_launch("rmem_label_tube_lineage");
}

extern "C" int rmem_label_tube_events(const unsigned char* labels, const int* roots, const int* links, int n, int H, int W, int* events,
                                      void* stream) {
  RMEM_REQUIRE(labels && roots && links && events, "rmem_label_tube_events: null pointer (labels, roots, links and events are required)");
  RMEM_TUBE_GEOMETRY("rmem_label_tube_events");
  const int HW = H * W;
  hipLaunchKernelGGL(k_tube_fill4, dim3(flat_blocks(256L * n)), dim3(kThreads), 0, (hipStream_t)stream, (int4*)events, (size_t)n * 256,
                     make_int4(0, 0, 0, 0));
  hipLaunchKernelGGL(k_tube_events, dim3(blocks_per_frame(16L * HW, n), n), dim3(kThreads), 0, (hipStream_t)stream, labels, roots, links, n, HW,
                     events);
  return rmem_check_launch("rmem_label_tube_events");
}

extern "C" int rmem_label_tube_index(const int* tubes, int n, int H, int W, int* rank, int* total, void* stream) {
  RMEM_REQUIRE(tubes && rank && total, "rmem_label_tube_index: null pointer (tubes, rank and total are required)");
  RMEM_TUBE_GEOMETRY("rmem_label_tube_index");
  const long long N = (long long)n * H * W;
  long long per_thread = (N + (long long)kThreads * kRankBlocks - 1) / ((long long)kThreads * kRankBlocks);
  if (per_thread < kRankPerThread) per_thread = kRankPerThread;
  const long long per = per_thread * kThreads;
  const int chunks = (int)((N + per - 1) / per);
  hipLaunchKernelGGL(k_tube_count, dim3(chunks), dim3(kThreads), 0, (hipStream_t)stream, tubes, (int)N, (int)per_thread, rank);
  hipLaunchKernelGGL(k_tube_scan, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, rank, chunks, (size_t)per, total);
  hipLaunchKernelGGL(k_tube_rank, dim3(chunks), dim3(kThreads), 0, (hipStream_t)stream, tubes, (int)N, (int)per_thread, rank);
  return rmem_check_launch("rmem_label_tube_index");
}

extern "C" int rmem_label_tube_table(const unsigned char* labels, const int* roots, const int* stats, const int* tubes, const int* rank, int n,
                                     int H, int W, int rows, int* table, void* stream) {
  RMEM_REQUIRE(labels && roots && stats && tubes && rank && table,
               "rmem_label_tube_table: null pointer (labels, roots, stats, tubes, rank and table are required)");
  RMEM_TUBE_GEOMETRY("rmem_label_tube_table");
  RMEM_REQUIRE(rows >= 0, "rmem_label_tube_table: rows must not be negative");
  if (rows == 0) return 0;                                          // a table without rows: nothing to write
  const int HW = H * W, N = n * HW;
  hipLaunchKernelGGL(k_tube_rows, dim3(flat_blocks(N)), dim3(kThreads), 0, (hipStream_t)stream, labels, tubes, rank, N, HW, rows, table);
  hipLaunchKernelGGL(k_tube_table, dim3(flat_blocks(N)), dim3(kThreads), 0, (hipStream_t)stream, roots, stats, tubes, rank, N, HW, rows, table);
  return rmem_check_launch("rmem_label_tube_table");
}

extern "C" int rmem_label_tube_clean(const unsigned char* src, unsigned char* dst, const int* roots, const int* stats, const int* tubes,
                                     const int* rank, const int* table, int n, int H, int W, int min_frames, int max_hole_frames, void* stream) {
  RMEM_REQUIRE(src && dst && roots && stats && tubes && rank && table,
               "rmem_label_tube_clean: null pointer (src, dst, roots, stats, tubes, rank and table are required)");
  RMEM_TUBE_GEOMETRY("rmem_label_tube_clean");
  RMEM_REQUIRE(min_frames >= 0 && max_hole_frames >= 0, "rmem_label_tube_clean: min_frames and max_hole_frames must not be negative");
  const int HW = H * W, N = n * HW;
  const TubeRule rule = {min_frames, max_hole_frames, n};
  hipLaunchKernelGGL(k_tube_clean, dim3(flat_blocks(N / 16 + 1)), dim3(kThreads), 0, (hipStream_t)stream, src, dst, roots, stats, tubes, rank,
                     table, HW, N, rule);
  return rmem_check_launch("rmem_label_tube_clean");
}
