// Geodesic nearest-site transform of uint8 label stacks over uint8 frames (include/rmem.h: rmem_label_geodesic_begin / _rounds /
// _finish; distance.py: geodesic_nearest, geodesic_grow).  The image-aware twin of label_nearest.hip: the same sites, the same three
// outputs, but the metric is the cheapest path through the 8-connected pixel grid whose edge between neighbours p and q costs
//   w(p, q) = spatial * s + colour * sum over the channels of |I_c(p) - I_c(q)|,   s = 5 for an axial step, 7 for a diagonal one.
// Integers only, bit-reproducible, independent of scheduling.  Element-type agnostic: built once.
//
// A KEY is 64 bits, (cost << 32) | flat index of the site: an unsigned compare is the lexicographic one.  kNoKey = (2^31 - 1, all
// ones) is "no site".  key(p) = the minimum over the sites s of (cheapest cost s -> p, index of s) is the one fixed point of
// "key(p) = min(key(p), key(q) + w(p, q)) over the eight neighbours q" that is reached from "kNoKey everywhere but (0, own index)
// on the sites": the system is monotone, so the order of relaxation, the tile and the number of rounds do not matter (DESIGN.md
// 8ac).  A candidate above the limit (max_cost, or 2^30 without one: above every real cost) is dropped where it arises: a prefix
// of a cheapest path is no dearer than the path.  So every key that is not kNoKey has a cost of at most 2^30, and the
// largest cost ever formed, kNoKey's 2^31 - 1 plus an edge, stays below 2^32: nothing overflows.
//
//   k_geo_begin    the first key plane from the labels and the site set.
//   k_geo_round    One workgroup per core tile of kTH x kTW pixels and frame.  It loads the tile's keys with a halo of one pixel
//                  (kNoKey outside the frame) from the source plane and the frame's pixels of the same region, relaxes inside LDS
//                  and stores the core to the OTHER plane: a round never writes what it reads, a tile's core is its neighbours' halo.
//                  A wave owns a band of kBand rows, a lane a column (kTW = 64).  Per pixel of its band the wave computes once per
//                  round the six weights to the rows above and below and P, the prefix sum of the row's horizontal weights from
//                  the left halo on (16 bytes per pixel in LDS).  A PASS: every wave reads the rows above and below its band,
//                  barrier, then sweeps its band down and up.  A row step takes the three keys of the row before (the lane's own
//                  and its neighbours' by wave shuffle, the halo columns from LDS), then runs the row's min-plus scans: to the
//                  right key[x] = min over j <= x of (key[j] - P[j]) + P[x], a prefix minimum of signed 64-bit values, and to the
//                  left the suffix minimum of key[j] + P[j].  In a pass a pixel's key in LDS is written by the one lane that owns
//                  it, and no wave reads another wave's rows between the two barriers of the pass.  A pass that lowers no key saw
//                  every relaxation of the core hold on the final values: the fixed point for this halo.  At most kCap passes: a
//                  tile that is still changing then reports "changed", so the cap only decides how many rounds it takes.
//                  Idle tiles: as k_thin_round's.  A tile whose own "changed" byte and whose eight neighbours' bytes of the round
//                  before are all 0 had, a round ago, the input it has now and did not change it: both planes hold its core, it
//                  writes a 0 byte and leaves.  The host passes those bytes from global round 1 on (round 0 reads the plane that
//                  begin wrote, and after it both planes hold every tile).
//   k_geo_finish   unpacks the final plane into index, cost and taken.
//
// No kernel waits for another workgroup, every loop is bounded, nothing is read or written beyond the frames, the outputs and the
// workspace.
#include <limits.h>
#include <stdlib.h>
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
constexpr int kTH = 32, kTW = 64;                  // core tile: a wave's lanes are the columns
constexpr int kRH = kTH + 2, kRW = kTW + 2;        // region: the core and a halo of one
constexpr int kBand = kTH / kWaves;                // rows of a wave
constexpr int kCap = 16;                           // passes of a round at most
constexpr int kMaxSide = 16384;
constexpr int kMaxCost = 1 << 30;                  // above every real cost: (kMaxSide - 1) * (64 * 7 + 64 * 765)
constexpr uint32_t kInf = 0x7fffffffu;
constexpr uint64_t kNoKey = ((uint64_t)kInf << 32) | 0xffffffffu;
static_assert(kTW == 64 && kTH % kWaves == 0 && (long)(kMaxSide - 1) * (64 * 7 + 64 * 765) < kMaxCost, "tile geometry, cost range");
static_assert(kRH * kRW * 8 + kRH * kRW * 4 + kTH * kTW * 16 + kTH * 4 <= 64 * 1024, "static LDS");

struct Bits256 {
  unsigned w[8];
};
__device__ __forceinline__ bool in_set(const Bits256& b, int v) { return (b.w[v >> 5] >> (v & 31)) & 1u; }

inline bool geo_geometry_ok(int n, int H, int W) { return stack_geometry_ok(n, H, W) && H <= kMaxSide && W <= kMaxSide; }
inline int geo_tiles(int H, int W, int& tiles_x) {
  tiles_x = (W + kTW - 1) / kTW;
  return (H + kTH - 1) / kTH;
}
inline size_t plane_bytes(int n, int H, int W) { return align16((size_t)n * H * W * 8); }

__global__ __launch_bounds__(kThreads) void k_geo_begin(const unsigned char* __restrict__ labels, int HW, Bits256 sites,
                                                        uint64_t* __restrict__ plane) {
  const size_t frame = (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < HW; p += gridDim.x * kThreads)
    plane[frame + p] = in_set(sites, labels[frame + p]) ? (uint64_t)(uint32_t)p : kNoKey;
}

__device__ __forceinline__ uint64_t kmin(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t kadd(uint64_t k, uint32_t w) { return k + ((uint64_t)w << 32); }   // kNoKey + w: above the limit, dropped
__device__ __forceinline__ uint32_t sad3(uint32_t a, uint32_t b) {
  return (uint32_t)(abs((int)(a & 0xffu) - (int)(b & 0xffu)) + abs((int)((a >> 8) & 0xffu) - (int)((b >> 8) & 0xffu)) +
                    abs((int)((a >> 16) & 0xffu) - (int)((b >> 16) & 0xffu)));
}

// the row's two min-plus scans; P: the lane's prefix sum of the horizontal weights.  (cost - P) may be negative: signed 64 bits,
// whose compare is the lexicographic one of (signed cost, unsigned index)
__device__ __forceinline__ uint64_t row_scans(uint64_t k, uint32_t P, int lane) {
  const long long p = (long long)((uint64_t)P << 32);
  const bool has = (uint32_t)(k >> 32) != kInf;    // k <= kNoKey here; "no key" takes no part: LLONG_MAX, which no sum reaches
  long long a = has ? (long long)k - p : LLONG_MAX, b = has ? (long long)k + p : LLONG_MAX;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long ua = __shfl_up(a, o, 64), ub = __shfl_down(b, o, 64);
    if (lane >= o && ua < a) a = ua;
    if (lane + o < 64 && ub < b) b = ub;
  }
  const uint64_t right = a == LLONG_MAX ? kNoKey : (uint64_t)(a + p), left = b == LLONG_MAX ? kNoKey : (uint64_t)(b - p);
  return kmin(k, kmin(right, left));
}

__global__ __launch_bounds__(kThreads) void k_geo_round(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                        const unsigned char* __restrict__ image, int C, int H, int W, int tiles_x,
                                                        int tiles_y, int spatial, int colour, uint32_t limit,
                                                        const unsigned char* __restrict__ idle, unsigned char* __restrict__ changed,
                                                        int* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) uint64_t key[kRH][kRW];
  __shared__ __attribute__((aligned(16))) uint4 wt[kTH][kTW];      // x = N | NW << 16, y = NE | S << 16, z = SW | SE << 16, w = P
  __shared__ uint32_t pix[kRH][kRW];                               // the pixel's channels, a byte each
  __shared__ uint32_t wright[kTH];                                 // the weight between a row's last core pixel and its right halo
  const int t = threadIdx.x, f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const size_t tiles = (size_t)tiles_x * tiles_y;
  const size_t tile = (size_t)f * tiles + blockIdx.x;
  if (idle) {                                      // the same nine bytes in every thread
    int any = 0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = ty + dy, xx = tx + dx;
        if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x) any |= idle[(size_t)f * tiles + (size_t)yy * tiles_x + xx];
      }
    if (!any) {
      if (t == 0) changed[tile] = 0;
      return;
    }
  }
  const size_t frame = (size_t)f * H * W;
  const int y0 = ty * kTH - 1, x0 = tx * kTW - 1;
  int fin = 0;
  for (int i = t; i < kRH * kRW; i += kThreads) {
    const int r = i / kRW, c = i - r * kRW;
    const int y = y0 + r, x = x0 + c;
    uint64_t k = kNoKey;
    uint32_t v = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t p = frame + (size_t)y * W + x;
      k = src[p];
      const unsigned char* px = image + p * C;
      v = px[0];
      if (C == 3) v |= ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    }
    key[r][c] = k;
    pix[r][c] = v;
    fin |= k != kNoKey;
  }
  const int live = __syncthreads_or(fin);          // the barrier too
  const int lane = t & 63, wave = t >> 6;
  const int r0 = 1 + wave * kBand, cc = lane + 1;  // the wave's first region row, the lane's region column
  int lowered = 0;
  if (live) {                                      // the same in every thread: a region without a key stays as it is
    for (int j = 0; j < kBand; ++j) {
      const int r = r0 + j;
      const uint32_t me = pix[r][cc];
      const uint32_t a = (uint32_t)spatial * 5u, d = (uint32_t)spatial * 7u, cw = (uint32_t)colour;
      const uint32_t wN = a + cw * sad3(me, pix[r - 1][cc]), wNW = d + cw * sad3(me, pix[r - 1][cc - 1]),
                     wNE = d + cw * sad3(me, pix[r - 1][cc + 1]), wS = a + cw * sad3(me, pix[r + 1][cc]),
                     wSW = d + cw * sad3(me, pix[r + 1][cc - 1]), wSE = d + cw * sad3(me, pix[r + 1][cc + 1]),
                     wW = a + cw * sad3(me, pix[r][cc - 1]);
      const uint32_t P = wave_incl_scan(wW, lane);
      wt[r - 1][lane] = make_uint4(wN | (wNW << 16), wNE | (wS << 16), wSW | (wSE << 16), P);
      if (lane == 63) wright[r - 1] = a + cw * sad3(me, pix[r][cc + 1]);
    }
    const bool colin = tx * kTW + lane < W;
    uint64_t seen_u = 0, seen_d = 0;               // the rows above and below at the wave's last sweep (0 is no key of a row)
    int mine = 1;                                  // the wave's last sweep lowered a key of its band (or there was none yet)
    for (int pass = 0; pass < kCap; ++pass) {
      // the rows above and below the band as they stand, before any wave writes
      const uint64_t ul = key[r0 - 1][cc - 1], um = key[r0 - 1][cc], ur = key[r0 - 1][cc + 1];
      const uint64_t dl = key[r0 + kBand][cc - 1], dm = key[r0 + kBand][cc], dr = key[r0 + kBand][cc + 1];
      __syncthreads();
      int ch = 0;
      // a band whose last sweep changed nothing and whose two rows are what that sweep saw is at its fixed point: the wave rests
      const bool sweep = __any(mine | (um != seen_u) | (dm != seen_d)) != 0;
      seen_u = um;
      seen_d = dm;
#pragma unroll 1
      for (int dir = 0; sweep && dir < 2; ++dir) {  // 0: down, from the row above; 1: up, from the row below
        uint64_t pl = dir ? dl : ul, pm = dir ? dm : um, pr = dir ? dr : ur;
#pragma unroll 1
        for (int j = 0; j < kBand; ++j) {
          const int r = dir ? r0 + kBand - 1 - j : r0 + j;
          const uint4 w = wt[r - 1][lane];
          const uint64_t old = key[r][cc];
          const uint64_t side = lane == 0 ? key[r][0] : (lane == 63 ? key[r][kRW - 1] : kNoKey);   // the halo columns: never written
          const uint32_t wl = dir ? (w.z & 0xffffu) : (w.x >> 16), wm = dir ? (w.y >> 16) : (w.x & 0xffffu),
                         wr = dir ? (w.z >> 16) : (w.y & 0xffffu);
          uint64_t k = kmin(kmin(old, kadd(pm, wm)), kmin(kadd(pl, wl), kadd(pr, wr)));
          const uint32_t wside = lane == 0 ? w.w : wright[r - 1];
          k = kmin(k, kadd(side, wside));
          k = row_scans(k, w.w, lane);
          const bool rowin = ty * kTH + r - 1 < H;
          if ((uint32_t)(k >> 32) > limit || !colin || !rowin) k = kNoKey;
          if (k != old) {
            key[r][cc] = k;
            ch = 1;
          }
          const uint64_t kl = __shfl_up((unsigned long long)k, 1, 64), kr = __shfl_down((unsigned long long)k, 1, 64);
          pl = lane == 0 ? side : kl;
          pm = k;
          pr = lane == 63 ? side : kr;
        }
      }
      mine = __any(ch) != 0;
      const int any = __syncthreads_or(ch);        // the barrier between two passes
      lowered |= any;
      if (!any) break;
    }
  }
  if (t == 0) {
    changed[tile] = lowered != 0;
    if (lowered && count) atomicAdd(count + f, 1);
  }
  for (int i = t; i < kTH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    const int y = ty * kTH + r, x = tx * kTW + c;
    if (y < H && x < W) dst[frame + (size_t)y * W + x] = key[r + 1][c + 1];
  }
}

__global__ __launch_bounds__(kThreads) void k_geo_finish(const unsigned char* __restrict__ labels, const uint64_t* __restrict__ plane, int HW,
                                                         Bits256 fill, uint32_t limit, int* __restrict__ index, int* __restrict__ cost,
                                                         unsigned char* __restrict__ taken) {
  const size_t frame = (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < HW; p += gridDim.x * kThreads) {
    const uint64_t k = plane[frame + p];
    const uint32_t c = (uint32_t)(k >> 32);
    const bool found = c <= limit;
    const int idx = found ? (int)(uint32_t)k : -1;
    if (index) index[frame + p] = idx;
    if (cost) cost[frame + p] = found ? (int)c : INT_MAX;
    if (taken) {
      const int me = labels[frame + p];
      taken[frame + p] = (found && in_set(fill, me)) ? labels[frame + idx] : (unsigned char)me;
    }
  }
}

inline int pixel_blocks(int HW, int n) {
  long b = ((long)HW + kThreads - 1) / kThreads;
  const long cap = kMaxBlocks / n > 1 ? kMaxBlocks / n : 1;
  return (int)(b > cap ? cap : b);
}
}  // namespace

#define RMEM_REQUIRE_GEO_STACK(fn, n, H, W)                                                      \
  RMEM_REQUIRE((n) >= 1 && (n) <= kMaxFrames, fn ": n must be in 1..65535");                     \
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), fn ": H and W must be positive, H * W at most 2^26"); \
  RMEM_REQUIRE((H) <= kMaxSide && (W) <= kMaxSide, fn ": H and W must be at most 16384")
#define RMEM_REQUIRE_GEO_WORKSPACE(fn, n, H, W, workspace, workspace_bytes)                                                      \
  RMEM_REQUIRE((workspace_bytes) >= rmem_label_geodesic_workspace_bytes(n, H, W),                                                \
               fn ": workspace too small (rmem_label_geodesic_workspace_bytes)");                                                \
  RMEM_REQUIRE(((uintptr_t)(workspace) & 15u) == 0, fn ": workspace must be 16-byte aligned")

extern "C" int rmem_label_geodesic_tile(int* th, int* tw) {
  RMEM_REQUIRE(th && tw, "rmem_label_geodesic_tile: null pointer");
  *th = kTH;
  *tw = kTW;
  return 0;
}

extern "C" long long rmem_label_geodesic_workspace_bytes(int n, int H, int W) {
  if (!geo_geometry_ok(n, H, W)) return 0;
  int tiles_x;
  const int tiles_y = geo_tiles(H, W, tiles_x);
  return 2 * (long long)plane_bytes(n, H, W) + 2 * (long long)align16((size_t)n * tiles_x * tiles_y);   // two key planes, two sets of tile bytes
}

extern "C" int rmem_label_geodesic_begin(const unsigned char* labels, int n, int H, int W, const unsigned int site_bits[8], void* workspace,
                                         long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(labels && site_bits && workspace, "rmem_label_geodesic_begin: null pointer (labels, site_bits and workspace are required)");
  RMEM_REQUIRE_GEO_STACK("rmem_label_geodesic_begin", n, H, W);
  RMEM_REQUIRE_GEO_WORKSPACE("rmem_label_geodesic_begin", n, H, W, workspace, workspace_bytes);
  Bits256 sites;
  for (int i = 0; i < 8; ++i) sites.w[i] = site_bits[i];
  hipLaunchKernelGGL(k_geo_begin, dim3(pixel_blocks(H * W, n), n), dim3(kThreads), 0, (hipStream_t)stream, labels, H * W, sites,
                     (uint64_t*)workspace);
  return rmem_check_launch("rmem_label_geodesic_begin");
}

extern "C" int rmem_label_geodesic_rounds(const unsigned char* image, int channels, int n, int H, int W, int spatial, int colour, int max_cost,
                                          int first_round, int count, int* changed, void* workspace, long long workspace_bytes,
                                          void* stream) {
  RMEM_REQUIRE(image && changed && workspace, "rmem_label_geodesic_rounds: null pointer (image, changed and workspace are required)");
  RMEM_REQUIRE(channels == 1 || channels == 3, "rmem_label_geodesic_rounds: channels must be 1 or 3");
  RMEM_REQUIRE_GEO_STACK("rmem_label_geodesic_rounds", n, H, W);
  RMEM_REQUIRE(spatial >= 1 && spatial <= 64, "rmem_label_geodesic_rounds: spatial must be in 1..64");
  RMEM_REQUIRE(colour >= 0 && colour <= 64, "rmem_label_geodesic_rounds: colour must be in 0..64");
  RMEM_REQUIRE(max_cost >= -1 && max_cost <= kMaxCost, "rmem_label_geodesic_rounds: max_cost must be -1 (no limit) or in 0..2^30");
  RMEM_REQUIRE(first_round >= 0, "rmem_label_geodesic_rounds: first_round must not be negative");
  RMEM_REQUIRE(count >= 1, "rmem_label_geodesic_rounds: count must be at least 1");
  RMEM_REQUIRE(first_round <= INT_MAX - count, "rmem_label_geodesic_rounds: first_round + count must fit 31 bits");
  RMEM_REQUIRE_GEO_WORKSPACE("rmem_label_geodesic_rounds", n, H, W, workspace, workspace_bytes);
  const hipStream_t st = (hipStream_t)stream;
  int tiles_x;
  const int tiles_y = geo_tiles(H, W, tiles_x);
  const size_t nt = (size_t)n * tiles_x * tiles_y, pb = plane_bytes(n, H, W);
  unsigned char* base = (unsigned char*)workspace;
  uint64_t* plane[2] = {(uint64_t*)base, (uint64_t*)(base + pb)};
  unsigned char* flags = base + 2 * pb;
  const size_t fb = align16(nt);
  const char* e = getenv("RMEM_GEODESIC_SKIP");     // read per call; 0: no tile is skipped (A/B runs, identity tests)
  const bool skip = !(e && atoi(e) == 0);
  if (hipMemsetAsync(changed, 0, (size_t)n * sizeof(int), st) != hipSuccess) {
    rmem_set_error("rmem_label_geodesic_rounds: hipMemsetAsync failed");
    return -1;
  }
  const uint32_t limit = max_cost < 0 ? (uint32_t)kMaxCost : (uint32_t)max_cost;
  for (int i = 0; i < count; ++i) {
    const int r = first_round + i;                 // round r reads plane r & 1 and the tile bytes of round r - 1, writes the others
    // a tile may be skipped once both planes hold it: from round 1 on, round 0 having read the plane begin wrote
    hipLaunchKernelGGL(k_geo_round, dim3(tiles_x * tiles_y, n), dim3(kThreads), 0, st, plane[r & 1], plane[(r + 1) & 1], image, channels, H, W,
                       tiles_x, tiles_y, spatial, colour, limit, (skip && r >= 1) ? flags + (size_t)((r - 1) & 1) * fb : (const unsigned char*)nullptr,
                       flags + (size_t)(r & 1) * fb, i == count - 1 ? changed : (int*)nullptr);
  }
  return rmem_check_launch("rmem_label_geodesic_rounds");
}

extern "C" int rmem_label_geodesic_finish(const unsigned char* labels, int n, int H, int W, const unsigned int fill_bits[8], int max_cost,
                                          int rounds, int* index, int* cost, unsigned char* taken, const void* workspace,
                                          long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(labels && workspace, "rmem_label_geodesic_finish: null pointer (labels and workspace are required)");
  RMEM_REQUIRE(index || cost || taken, "rmem_label_geodesic_finish: no output (at least one of index, cost and taken is required)");
  RMEM_REQUIRE(taken != labels, "rmem_label_geodesic_finish: taken must not be labels (labels are read at the winning site while taken is written)");
  RMEM_REQUIRE_GEO_STACK("rmem_label_geodesic_finish", n, H, W);
  RMEM_REQUIRE(max_cost >= -1 && max_cost <= kMaxCost, "rmem_label_geodesic_finish: max_cost must be -1 (no limit) or in 0..2^30");
  RMEM_REQUIRE(rounds >= 0, "rmem_label_geodesic_finish: rounds must not be negative");
  RMEM_REQUIRE_GEO_WORKSPACE("rmem_label_geodesic_finish", n, H, W, workspace, workspace_bytes);
  Bits256 fill;
  for (int i = 0; i < 8; ++i) fill.w[i] = fill_bits ? fill_bits[i] : 0xffffffffu;
  const uint64_t* plane = (const uint64_t*)((const unsigned char*)workspace + (size_t)(rounds & 1) * plane_bytes(n, H, W));
  const uint32_t limit = max_cost < 0 ? (uint32_t)kMaxCost : (uint32_t)max_cost;
  hipLaunchKernelGGL(k_geo_finish, dim3(pixel_blocks(H * W, n), n), dim3(kThreads), 0, (hipStream_t)stream, labels, plane, H * W, fill, limit,
                     index, cost, taken);
  return rmem_check_launch("rmem_label_geodesic_finish");
}
