// Thinning of uint8 label stacks to skeletons (Guo and Hall 1989, algorithm A1) and the list of a stack's non-zero pixels
// (include/rmem.h: rmem_label_thin, rmem_label_pixels_count, rmem_label_pixels_write; skeleton.py).  Bytes in, bytes out, integers
// only: the result is bit-identical to the host restatement.  Element-type agnostic: built once.
//
// The rule.  A pixel p of value L != 0 sees eight neighbour bits x1..x8 = E, NE, N, NW, W, SW, S, SE (y grows
// downward), x_i = 1 iff that neighbour lies inside the frame and holds L; mask bit k = x_{k+1}.  p is deleted in a sub-iteration
// iff the sub-iteration's 256-entry table holds its mask; even sub-iterations use table 0, odd ones table 1.  Every value is
// thinned as if it were alone in the frame.  A sub-iteration is synchronous.
//
//   k_thin_round   One workgroup per core tile of kTH x kTW pixels and frame.  It loads the core plus a halo of kK pixels (zeros
//                  outside the frame) into LDS as words of four pixels, runs up to kK sub-iterations there, ping-ponging two LDS
//                  planes with a barrier in between, and stores the core alone.  The region evolves as a frame of its own, so after
//                  s sub-iterations everything farther than s pixels from its rim is exact: the core is exact after kK.  kK is
//                  even: every full round starts at the same parity.  A thread takes words t, t + 256, ...: a zero word costs one
//                  LDS read, another one nine reads and a table bit per non-zero pixel.  The barrier is a workgroup-wide OR of
//                  "deleted something": two quiet sub-iterations in a row are a fixed point of the region and end the round.
//                  Idle tiles: every round writes one "changed" byte per tile (its core lost a pixel).  A tile whose own byte and
//                  whose eight neighbours' bytes of the round before are all 0 writes a 0 byte and leaves: its input is what it
//                  was a round before, so is the parity, the output was the input, and both global buffers hold it already.  The
//                  host passes those bytes only from the round on at which both buffers do hold every tile.
//                  lost: deleted core pixels, summed per wave, then per workgroup in LDS, one integer atomic per workgroup and word.
//   k_pixels_count, k_label_scan_units (label_scan.h), k_pixels_bases, k_pixels_write
//                  The count-then-write of rle.hip: a unit is kUnit consecutive pixels of a frame, 16 per thread; the counters are
//                  scanned per frame, the frames' totals to 64-bit bases, and the second walk writes (frame, y, x, value) in
//                  raster order, with the value of an int32 stack at each listed pixel if one is given.
//
// No kernel waits for another workgroup, every loop is bounded, nothing is read or written beyond [0, H) x [0, W) of a frame.
#include <limits.h>
#include <stdlib.h>
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
constexpr int kTH = 48, kTW = 112, kK = 8;         // core tile, halo = sub-iterations per launch
constexpr int kRH = kTH + 2 * kK;                  // region rows (64)
constexpr int kRWW = (kTW + 2 * kK) / 4;           // region words per row (32): a row is one word per LDS bank
constexpr int kRegion = kRH * kRWW;                // 2048 words, 8 per thread
constexpr int kCoreWW = kTW / 4;
static_assert(kK % 2 == 0 && kK % 4 == 0 && kTW % 4 == 0 && kRWW == 32 && kRegion % kThreads == 0, "tile geometry");
constexpr int kUnit = kThreads * 16;               // pixels of one unit of the pixel list

struct ThinTables {
  uint32_t w[16];                                  // [parity][8]: bit m of table parity = a pixel with mask m is deleted
};

constexpr bool thin_deletes(int m, int parity) {
  int x[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 8; ++k) x[k + 1] = (m >> k) & 1;
  x[9] = x[1];
  int xh = 0, n1 = 0, n2 = 0;
  for (int i = 1; i <= 4; ++i) {
    xh += (x[2 * i - 1] == 0 && (x[2 * i] == 1 || x[2 * i + 1] == 1)) ? 1 : 0;
    n1 += x[2 * i - 1] | x[2 * i];
    n2 += x[2 * i] | x[2 * i + 1];
  }
  const int mn = n1 < n2 ? n1 : n2;
  const bool g3 = parity == 0 ? (((x[2] | x[3] | (1 - x[8])) & x[1]) == 0) : (((x[6] | x[7] | (1 - x[4])) & x[5]) == 0);
  return xh == 1 && mn >= 2 && mn <= 3 && g3;
}
constexpr ThinTables make_tables() {
  ThinTables t = {};
  for (int p = 0; p < 2; ++p)
    for (int m = 0; m < 256; ++m)
      if (thin_deletes(m, p)) t.w[p * 8 + (m >> 5)] |= 1u << (m & 31);
  return t;
}
constexpr ThinTables kHostTables = make_tables();  // one constant expression: the host's export and the device's copy
__constant__ ThinTables kDeviceTables = make_tables();

// four pixels of a row from x (any sign) as one word, zeros outside [0, W); row: the row's first byte
__device__ __forceinline__ uint32_t load_word(const unsigned char* row, int x, int W) {
  if (x >= 0 && x + 3 < W) {
    const unsigned char* p = row + x;
    if (((uintptr_t)p & 3u) == 0) return *(const uint32_t*)p;
    return load4(p);
  }
  uint32_t w = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (x + b >= 0 && x + b < W) w |= (uint32_t)row[x + b] << (8 * b);
  return w;
}
__device__ __forceinline__ void store_word(unsigned char* row, int x, int W, uint32_t w) {
  unsigned char* p = row + x;
  if (x + 3 < W && ((uintptr_t)p & 3u) == 0) {
    *(uint32_t*)p = w;
    return;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (x + b < W) p[b] = (unsigned char)(w >> (8 * b));
}

// a row's three words as the six bytes a word's four pixels see: byte 0 the pixel left of the word, byte 5 the one right of it
__device__ __forceinline__ uint64_t window(uint32_t l, uint32_t m, uint32_t r) {
  return (uint64_t)(l >> 24) | ((uint64_t)m << 8) | ((uint64_t)(r & 0xffu) << 40);
}

__global__ __launch_bounds__(kThreads) void k_thin_round(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H, int W,
                                                         int tiles_x, int tiles_y, int nsub, int parity, int tail_from,
                                                         const unsigned char* __restrict__ idle, unsigned char* __restrict__ changed,
                                                         int* __restrict__ lost) {
  __shared__ uint32_t plane[2][kRegion];
  __shared__ uint32_t stab[16];
  __shared__ int scount[2];
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
  const int y0 = ty * kTH - kK, x0 = tx * kTW - kK;
  uint32_t nz = 0;
#pragma unroll
  for (int i = t; i < kRegion; i += kThreads) {
    const int y = y0 + (i >> 5), x = x0 + 4 * (i & 31);
    uint32_t w = 0;
    if (y >= 0 && y < H && x + 3 >= 0 && x < W) w = load_word(src + frame + (size_t)y * W, x, W);
    plane[0][i] = w;
    nz |= w;
  }
  if (t < 16) stab[t] = kDeviceTables.w[t];
  if (t < 2) scount[t] = 0;
  const int live = __syncthreads_or(nz != 0);      // the barrier too
  int cur = 0, lost_all = 0, lost_tail = 0;
  if (live) {
    int quiet = 0;
    for (int s = 0; s < nsub; ++s) {
      const uint32_t* A = plane[cur];
      uint32_t* B = plane[cur ^ 1];
      const uint32_t* T = stab + ((parity + s) & 1) * 8;
      int deleted = 0;
#pragma unroll
      for (int i = t; i < kRegion; i += kThreads) {
        const uint32_t m = A[i];
        uint32_t o = m;
        if (m) {
          const int r = i >> 5, c = i & 31;
          const bool up = r > 0, down = r < kRH - 1, left = c > 0, right = c < kRWW - 1;
          const uint64_t wu = up ? window(left ? A[i - 33] : 0u, A[i - 32], right ? A[i - 31] : 0u) : 0ull;
          const uint64_t wm = window(left ? A[i - 1] : 0u, m, right ? A[i + 1] : 0u);
          const uint64_t wd = down ? window(left ? A[i + 31] : 0u, A[i + 32], right ? A[i + 33] : 0u) : 0ull;
          int d = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t L = (m >> (8 * j)) & 0xffu;
            if (L) {
              const uint32_t u0 = (uint32_t)(wu >> (8 * j)) & 0xffu, u1 = (uint32_t)(wu >> (8 * j + 8)) & 0xffu,
                             u2 = (uint32_t)(wu >> (8 * j + 16)) & 0xffu;
              const uint32_t m0 = (uint32_t)(wm >> (8 * j)) & 0xffu, m2 = (uint32_t)(wm >> (8 * j + 16)) & 0xffu;
              const uint32_t d0 = (uint32_t)(wd >> (8 * j)) & 0xffu, d1 = (uint32_t)(wd >> (8 * j + 8)) & 0xffu,
                             d2 = (uint32_t)(wd >> (8 * j + 16)) & 0xffu;
              const uint32_t mask = (uint32_t)(m2 == L) | ((uint32_t)(u2 == L) << 1) | ((uint32_t)(u1 == L) << 2) |
                                    ((uint32_t)(u0 == L) << 3) | ((uint32_t)(m0 == L) << 4) | ((uint32_t)(d0 == L) << 5) |
                                    ((uint32_t)(d1 == L) << 6) | ((uint32_t)(d2 == L) << 7);
              if ((T[mask >> 5] >> (mask & 31)) & 1u) {
                o &= ~(0xffu << (8 * j));
                ++d;
              }
            }
          }
          if (d) {
            deleted = 1;
            if (r >= kK && r < kK + kTH && c >= kK / 4 && c < kK / 4 + kCoreWW) {       // the core: exact in every sub-iteration
              lost_all += d;
              if (s >= tail_from) lost_tail += d;
            }
          }
        }
        B[i] = o;
      }
      const int any = __syncthreads_or(deleted);   // the barrier between two sub-iterations
      cur ^= 1;
      quiet = any ? 0 : quiet + 1;
      if (quiet == 2) break;                       // a fixed point of the region: the rest of the round changes nothing
    }
    lost_all = wave_isum(lost_all);
    lost_tail = wave_isum(lost_tail);
    if ((t & 63) == 0) {
      if (lost_all) atomicAdd(&scount[0], lost_all);
      if (lost_tail) atomicAdd(&scount[1], lost_tail);
    }
    __syncthreads();
  }
  if (t == 0) {
    const int all = live ? scount[0] : 0, tail = live ? scount[1] : 0;
    if (all) atomicAdd(lost + 2 * f, all);
    if (tail) atomicAdd(lost + 2 * f + 1, tail);
    changed[tile] = all != 0;
  }
  const uint32_t* P = plane[cur];
  for (int i = t; i < kTH * kCoreWW; i += kThreads) {
    const int r = i / kCoreWW, c = i - r * kCoreWW;
    const int y = ty * kTH + r, x = tx * kTW + 4 * c;
    if (y < H && x < W) store_word(dst + frame + (size_t)y * W, x, W, P[(r + kK) * kRWW + c + kK / 4]);
  }
}

// ----------------------------------------------------------------------------------------------------------- pixel list
__device__ __forceinline__ int unit_pixels(const unsigned char* F, int p0, int HW, unsigned char (&v)[16]) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] = p0 + j < HW ? F[p0 + j] : (unsigned char)0;
    c += v[j] != 0;
  }
  return c;
}

__global__ __launch_bounds__(kThreads) void k_pixels_count(const unsigned char* __restrict__ stack, int HW, int U, int* __restrict__ cnt) {
  __shared__ int sh[kWaves];
  const int t = threadIdx.x, f = blockIdx.y, u = blockIdx.x;
  unsigned char v[16];
  const int c = wave_isum(unit_pixels(stack + (size_t)f * HW, u * kUnit + t * 16, HW, v));
  if ((t & 63) == 0) sh[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += sh[k];
    cnt[(size_t)f * U + u] = s;
  }
}

// one workgroup: bases[f] = the pixels listed before frame f, 64 bits
__global__ __launch_bounds__(kThreads) void k_pixels_bases(const int* __restrict__ totals, int n, long long* __restrict__ bases) {
  __shared__ long long sh[kWaves];
  long long carry = 0;
  for (int b = 0; b < n; b += kThreads) {
    const int i = b + threadIdx.x;
    const long long v = i < n ? totals[i] : 0;
    long long tot;
    const long long inc = block_incl_scan(v, sh, tot);
    if (i < n) bases[i] = carry + inc - v;
    carry += tot;
  }
}

__global__ __launch_bounds__(kThreads) void k_pixels_write(const unsigned char* __restrict__ stack, const int* __restrict__ samples, int HW,
                                                           int W, int U, const int* __restrict__ cnt, const long long* __restrict__ bases,
                                                           long long capacity, int* __restrict__ entries, int* __restrict__ sampled) {
  __shared__ int sh[kWaves];
  const int t = threadIdx.x, f = blockIdx.y, u = blockIdx.x;
  const int p0 = u * kUnit + t * 16;
  unsigned char v[16];
  const int c = unit_pixels(stack + (size_t)f * HW, p0, HW, v);
  int tot;
  const int inc = block_incl_scan(c, sh, tot);
  if (!c) return;                                  // after the scan's barriers
  long long row = bases[f] + cnt[(size_t)f * U + u] + (inc - c);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (v[j] && row < capacity) {
      const int p = p0 + j, y = p / W;
      int* e = entries + row * 4;
      e[0] = f;
      e[1] = y;
      e[2] = p - y * W;
      e[3] = v[j];
      if (samples) sampled[row] = samples[(size_t)f * HW + p];
    }
    row += v[j] != 0;
  }
}

inline int thin_tiles(int H, int W, int& tiles_x) {
  tiles_x = (W + kTW - 1) / kTW;
  return (H + kTH - 1) / kTH;
}
inline int pixel_units(int H, int W) { return (int)(((long)H * W + kUnit - 1) / kUnit); }
}  // namespace

extern "C" int rmem_label_thin_tile(int* th, int* tw, int* k) {
  RMEM_REQUIRE(th && tw && k, "rmem_label_thin_tile: null pointer");
  *th = kTH;
  *tw = kTW;
  *k = kK;
  return 0;
}

extern "C" int rmem_label_thin_table(int parity, unsigned char* out) {
  RMEM_REQUIRE(out, "rmem_label_thin_table: null pointer");
  RMEM_REQUIRE(parity == 0 || parity == 1, "rmem_label_thin_table: parity must be 0 or 1");
  for (int b = 0; b < 32; ++b) out[b] = (unsigned char)(kHostTables.w[parity * 8 + b / 4] >> (8 * (b & 3)));
  return 0;
}

extern "C" long long rmem_label_thin_workspace_bytes(int n, int H, int W) {
  if (!stack_geometry_ok(n, H, W)) return 0;
  int tiles_x;
  const int tiles_y = thin_tiles(H, W, tiles_x);
  return (long long)align16((size_t)n * H * W) + (long long)align16(2 * (size_t)n * tiles_x * tiles_y);   // the second stack, two sets of tile bytes
}

extern "C" int rmem_label_thin(const unsigned char* labels, int n, int H, int W, int first, int count, unsigned char* out, int* lost,
                               void* workspace, long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(labels && out && lost && workspace, "rmem_label_thin: null pointer (labels, out, lost and workspace are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_thin: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_thin: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(first >= 0, "rmem_label_thin: first must not be negative");
  RMEM_REQUIRE(count >= 1, "rmem_label_thin: count must be at least 1");
  RMEM_REQUIRE(first <= INT_MAX - count, "rmem_label_thin: first + count must fit 31 bits");
  RMEM_REQUIRE(workspace_bytes >= rmem_label_thin_workspace_bytes(n, H, W), "rmem_label_thin: workspace too small (rmem_label_thin_workspace_bytes)");
  RMEM_REQUIRE(((uintptr_t)workspace & 3u) == 0, "rmem_label_thin: workspace must be 4-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n * H * W;
  int tiles_x;
  const int tiles_y = thin_tiles(H, W, tiles_x);
  const size_t nt = (size_t)n * tiles_x * tiles_y;
  unsigned char* other = (unsigned char*)workspace;
  unsigned char* flags = other + align16(bytes);
  const char* e = getenv("RMEM_THIN_SKIP");         // read per call; 0: no tile is skipped (A/B runs, identity tests)
  const bool skip = !(e && atoi(e) == 0);
  if (hipMemsetAsync(lost, 0, (size_t)n * 2 * sizeof(int), st) != hipSuccess) {
    rmem_set_error("rmem_label_thin: hipMemsetAsync failed");
    return -1;
  }
  // round r writes `out` where an even number of rounds follow it, else the workspace's stack: the last round lands in out.  A
  // round must not write what it reads (a tile's core is another tile's halo): in place with an odd number of rounds the first
  // round reads a copy.
  const int rounds = (count + kK - 1) / kK;
  const unsigned char* src = labels;
  if ((rounds & 1) && labels == out) {
    if (hipMemcpyAsync(other, labels, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      rmem_set_error("rmem_label_thin: hipMemcpyAsync failed");
      return -1;
    }
    src = other;
  }
  const unsigned char* src0 = src;
  const int tail_start = count >= 2 ? count - 2 : 0;                // the call's last two sub-iterations count into lost[f][1]
  for (int r = 0; r < rounds; ++r) {
    unsigned char* dst = ((rounds - 1 - r) & 1) ? other : out;
    const int s0 = r * kK, nsub = count - s0 < kK ? count - s0 : kK;
    int tail_from = tail_start - s0;
    tail_from = tail_from < 0 ? 0 : (tail_from > nsub ? nsub : tail_from);
    // a tile may be skipped once the buffer this round writes held it a round ago: from the third round on, in the second one
    // if the first read the buffer the second writes
    const bool both = r >= 2 || (r == 1 && src0 == dst);
    hipLaunchKernelGGL(k_thin_round, dim3(tiles_x * tiles_y, n), dim3(kThreads), 0, st, src, dst, H, W, tiles_x, tiles_y, nsub, first & 1,
                       tail_from, (skip && both) ? flags + (size_t)((r - 1) & 1) * nt : (const unsigned char*)nullptr,
                       flags + (size_t)(r & 1) * nt, lost);
    src = dst;
  }
  return rmem_check_launch("rmem_label_thin");
}

extern "C" long long rmem_label_pixels_workspace_bytes(int n, int H, int W) {
  if (!stack_geometry_ok(n, H, W)) return 0;
  return (long long)align16((size_t)n * 8) + (long long)align16((size_t)n * pixel_units(H, W) * 4);   // the frames' bases, the unit counters
}

extern "C" int rmem_label_pixels_count(const unsigned char* stack, int n, int H, int W, int* totals, void* workspace, long long workspace_bytes,
                                       void* stream) {
  RMEM_REQUIRE(stack && totals && workspace, "rmem_label_pixels_count: null pointer (stack, totals and workspace are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_pixels_count: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_pixels_count: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(workspace_bytes >= rmem_label_pixels_workspace_bytes(n, H, W),
               "rmem_label_pixels_count: workspace too small (rmem_label_pixels_workspace_bytes)");
  RMEM_REQUIRE(((uintptr_t)workspace & 7u) == 0, "rmem_label_pixels_count: workspace must be 8-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int U = pixel_units(H, W);
  long long* bases = (long long*)workspace;
  int* cnt = (int*)((unsigned char*)workspace + align16((size_t)n * 8));
  hipLaunchKernelGGL(k_pixels_count, dim3(U, n), dim3(kThreads), 0, st, stack, H * W, U, cnt);
  hipLaunchKernelGGL(k_label_scan_units, dim3(n), dim3(kThreads), 0, st, cnt, U, totals);
  hipLaunchKernelGGL(k_pixels_bases, dim3(1), dim3(kThreads), 0, st, totals, n, bases);
  return rmem_check_launch("rmem_label_pixels_count");
}

extern "C" int rmem_label_pixels_write(const unsigned char* stack, const int* samples, int n, int H, int W, long long capacity, int* entries,
                                       int* sampled, const void* workspace, long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(stack && entries && workspace, "rmem_label_pixels_write: null pointer (stack, entries and workspace are required)");
  RMEM_REQUIRE((samples == nullptr) == (sampled == nullptr), "rmem_label_pixels_write: samples and sampled go together");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_pixels_write: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_pixels_write: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(capacity >= 0, "rmem_label_pixels_write: capacity must not be negative");
  RMEM_REQUIRE(workspace_bytes >= rmem_label_pixels_workspace_bytes(n, H, W),
               "rmem_label_pixels_write: workspace too small (rmem_label_pixels_workspace_bytes)");
  RMEM_REQUIRE(((uintptr_t)workspace & 7u) == 0, "rmem_label_pixels_write: workspace must be 8-byte aligned");
  const int U = pixel_units(H, W);
  const long long* bases = (const long long*)workspace;
  const int* cnt = (const int*)((const unsigned char*)workspace + align16((size_t)n * 8));
  hipLaunchKernelGGL(k_pixels_write, dim3(U, n), dim3(kThreads), 0, (hipStream_t)stream, stack, samples, H * W, W, U, cnt, bases, capacity,
                     entries, sampled);
  return rmem_check_launch("rmem_label_pixels_write");
}
