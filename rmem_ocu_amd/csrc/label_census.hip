// Label census and label remap (include/rmem.h, rmem_label_census / rmem_label_remap): what turns a decoded annotation stack into
// the clip protocol of protocol.py -- which ids a frame holds, how large they are and where (census), and the renumbering of
// sparse palette ids, the first-frame label and the new-object overlays (remap with one 256-entry table per frame).
// Element-type agnostic (uint8 in, int32 / uint8 out): built once.
//
//   k_census   A frame is a flat range of H * W bytes that may start at any byte: single bytes up to the first 16-byte boundary
//              (head) and after the last one (tail), one 16-byte load per lane in between.  A lane never adds a pixel to LDS on
//              its own -- label maps are long runs of one value, 64 lanes would queue on one address.  Per wave, for every
//              distinct value v among the lanes' bytes (picked from the first lane that still has bytes left): each lane's 16-bit
//              mask of its bytes equal to v, the mask's area and box, the wave's totals, one LDS update by five lanes.  Lanes
//              are in frame order, so the first and the last lane with a hit give the y range (and the x range when that is one
//              row); wave reductions remain for the area of partly covered lanes and the x range over several rows.  A lane
//              whose 16 bytes are all equal compares one byte instead of 16; a wave whose 1024 bytes are all equal is one run
//              and needs no reduction at all.  Per workgroup the tables (area, xmin, ymin, xmax, ymax) x 256 live in LDS and
//              their non-empty entries are flushed with integer global atomics (add / min / max): the result does not depend on
//              the order of arrival.  k_census_init writes the "absent" entry (0, W, H, -1, -1) everywhere first.
//   k_remap    The frame's 256-byte table is staged in LDS; 16-byte stores where dst allows them, 16-byte loads where src allows
//              them at the same offsets (always, in place), single bytes at head and tail.
#include <limits.h>
#include "label_wave.h"
#include "../../include/rmem.h"

namespace {
__device__ __forceinline__ int top_bit(unsigned m) { return 31 - __builtin_clz(m); }

// Box of the bytes in m (non-zero, 16 bits): byte j is the pixel j steps after (y, x) in a row-major image W wide.
__device__ __forceinline__ void box_of(unsigned m, int y, int x, int W, int& x0, int& y0, int& x1, int& y1) {
  const int lo = __builtin_ctz(m), hi = top_bit(m);
  if (x + hi < W) {                    // one image row
    x0 = x + lo; x1 = x + hi; y0 = y1 = y;
    return;
  }
  if (W >= 16) {                       // two rows: bytes below j0 on row y, the rest on row y + 1 from x = 0
    const int j0 = W - x;              // 1 <= j0 <= hi
    const unsigned ml = m & ((1u << j0) - 1u), mh = m >> j0;
    x0 = __builtin_ctz(mh); x1 = top_bit(mh); y0 = y1 = y + 1;
    if (ml) {
      y0 = y;
      x0 = min(x0, x + __builtin_ctz(ml));
      x1 = max(x1, x + top_bit(ml));
    }
    return;
  }
  x0 = y0 = INT_MAX; x1 = y1 = -1;     // rows shorter than a load: walk the bytes
  int yy = y, xx = x;
  for (int j = 0; j <= hi; ++j) {
    if ((m >> j) & 1u) {
      x0 = min(x0, xx); x1 = max(x1, xx);
      y0 = min(y0, yy); y1 = yy;
    }
    if (++xx == W) { xx = 0; ++yy; }
  }
}

__device__ __forceinline__ void table_update(int (*tab)[256], int lane, int v, int area, int x0, int y0, int x1, int y1) {
  if (lane == 0) atomicAdd(&tab[0][v], area);
  else if (lane == 1) atomicMin(&tab[1][v], x0);
  else if (lane == 2) atomicMin(&tab[2][v], y0);
  else if (lane == 3) atomicMax(&tab[3][v], x1);
  else if (lane == 4) atomicMax(&tab[4][v], y1);
}

// One wave's step: lane l holds the bytes `rem` (a 16-bit mask; 0 = nothing) of w, byte 0 at pixel (y, x).  Lanes hold
// consecutive pieces of the frame in lane order.  Called by whole waves only.
__device__ __forceinline__ void wave_census(uint4 w, unsigned rem, int y, int x, int W, int lane, int (*tab)[256]) {
  const bool uni = rem == 0xffffu && all_equal(w);
  const int first = (int)(w.x & 0xffu);
  if (__ballot(uni) == ~0ull) {
    const int v = __builtin_amdgcn_readfirstlane(first);
    if (__ballot(first == v) == ~0ull) {           // the wave's 1024 bytes are one run of v starting at lane 0's pixel
      const int ys = __builtin_amdgcn_readfirstlane(y), xs = __builtin_amdgcn_readfirstlane(x);
      const int xe = xs + 64 * 16 - 1;
      const bool one_row = xe < W;
      table_update(tab, lane, v, 64 * 16, one_row ? xs : 0, ys, one_row ? xe : W - 1, one_row ? ys : ys + xe / W);
      return;
    }
  }
  for (;;) {
    const uint64_t busy = __ballot(rem != 0);
    if (!busy) break;
    const int cand = byte_at(w, rem ? __builtin_ctz(rem) : 0);
    const int v = __builtin_amdgcn_readlane(cand, __builtin_ctzll(busy));
    unsigned m;
    if (uni) {
      m = first == v ? 0xffffu : 0u;               // the cheap path: one compare for 16 equal bytes
    } else {
      const uint32_t v4 = (uint32_t)v * 0x01010101u;
      m = (eq4(w.x, v4) | (eq4(w.y, v4) << 4) | (eq4(w.z, v4) << 8) | (eq4(w.w, v4) << 12)) & rem;
    }
    rem &= ~m;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    if (m) box_of(m, y, x, W, x0, y0, x1, y1);
    // Lanes hold the frame in lane order, so the first lane with a hit has the smallest y and the last one the largest, and when
    // those are one row the same holds for x: reductions are left for the area of partly covered lanes and the x of several rows.
    const uint64_t hit = __ballot(m != 0);         // never empty: the lane v was picked from holds it
    const int lo = __builtin_ctzll(hit), hi = 63 - __builtin_clzll(hit);
    const int area = __ballot(m == 0xffffu) == hit ? 16 * __popcll(hit) : wave_isum(__popc(m));
    y0 = __builtin_amdgcn_readlane(y0, lo);
    y1 = __builtin_amdgcn_readlane(y1, hi);
    if (y0 == y1) {
      x0 = __builtin_amdgcn_readlane(x0, lo);
      x1 = __builtin_amdgcn_readlane(x1, hi);
    } else {
      x0 = wave_imin(x0);
      x1 = wave_imax(x1);
    }
    table_update(tab, lane, v, area, x0, y0, x1, y1);
  }
}

__global__ __launch_bounds__(kThreads) void k_census_init(int* __restrict__ out, int entries, int H, int W) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= entries) return;
  int* o = out + (size_t)i * 5;
  o[0] = 0; o[1] = W; o[2] = H; o[3] = -1; o[4] = -1;
}

__global__ __launch_bounds__(kThreads) void k_census(const unsigned char* __restrict__ labels, int HW, int W, int* __restrict__ out) {
  __shared__ int tab[5][256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  tab[0][t] = 0; tab[1][t] = INT_MAX; tab[2][t] = INT_MAX; tab[3][t] = -1; tab[4][t] = -1;
  __syncthreads();
  const int f = blockIdx.y;
  const unsigned char* base = labels + (size_t)f * HW;
  int head = (int)((16u - (unsigned)((uintptr_t)base & 15u)) & 15u);
  if (head > HW) head = HW;
  const int nchunks = (HW - head) >> 4;
  const int tail_begin = head + 16 * nchunks, tail = HW - tail_begin;
  for (int c0 = (blockIdx.x * kWaves + wave) * 64; c0 < nchunks; c0 += gridDim.x * kThreads) {
    const int c = c0 + lane;
    uint4 w = make_uint4(0, 0, 0, 0);
    unsigned rem = 0;
    int y = 0, x = 0;
    if (c < nchunks) {
      const int p = head + 16 * c;
      w = *(const uint4*)(base + p);
      rem = 0xffffu;
      y = p / W; x = p - y * W;
    }
    wave_census(w, rem, y, x, W, lane, tab);
  }
  if (blockIdx.x == 0 && wave == 0 && head + tail > 0) {       // lanes 0..14: the head's bytes, lanes 16..30: the tail's
    int p = -1;
    if (lane < head) p = lane;
    else if (lane >= 16 && lane - 16 < tail) p = tail_begin + lane - 16;
    uint4 w = make_uint4(0, 0, 0, 0);
    unsigned rem = 0;
    int y = 0, x = 0;
    if (p >= 0) {
      w.x = base[p];
      rem = 1u;
      y = p / W; x = p - y * W;
    }
    wave_census(w, rem, y, x, W, lane, tab);
  }
  __syncthreads();
  const int area = tab[0][t];
  if (area) {
    int* o = out + ((size_t)f * 256 + t) * 5;
    atomicAdd(o + 0, area);
    atomicMin(o + 1, tab[1][t]);
    atomicMin(o + 2, tab[2][t]);
    atomicMax(o + 3, tab[3][t]);
    atomicMax(o + 4, tab[4][t]);
  }
}

__device__ __forceinline__ uint32_t map4(uint32_t w, const unsigned char* lut) {
  return (uint32_t)lut[w & 0xffu] | ((uint32_t)lut[(w >> 8) & 0xffu] << 8) | ((uint32_t)lut[(w >> 16) & 0xffu] << 16) |
         ((uint32_t)lut[w >> 24] << 24);
}

// src and dst may be the same frame: every byte is read and written by the same thread, and read first.
__global__ __launch_bounds__(kThreads) void k_remap(const unsigned char* src, unsigned char* dst, int pixels, const unsigned char* __restrict__ luts,
                                                    int lut_per_frame) {
  __shared__ __attribute__((aligned(16))) unsigned char lut[256];
  const int t = threadIdx.x, f = blockIdx.y;
  lut[t] = luts[(size_t)(lut_per_frame ? f : 0) * 256 + t];
  __syncthreads();
  const unsigned char* s = src + (size_t)f * pixels;
  unsigned char* d = dst + (size_t)f * pixels;
  int head = (int)((16u - (unsigned)((uintptr_t)d & 15u)) & 15u);
  if (head > pixels) head = pixels;
  const int nchunks = (pixels - head) >> 4;
  const int tail_begin = head + 16 * nchunks, tail = pixels - tail_begin;
  const bool src_wide = (((uintptr_t)s + head) & 15u) == 0;      // uniform per frame
  for (int c = blockIdx.x * kThreads + t; c < nchunks; c += gridDim.x * kThreads) {
    const int p = head + 16 * c;
    uint4 w;
    if (src_wide) w = *(const uint4*)(s + p);
    else w = make_uint4(load4(s + p), load4(s + p + 4), load4(s + p + 8), load4(s + p + 12));
    uint4 o;
    if (all_equal(w)) {
      const uint32_t r = (uint32_t)lut[w.x & 0xffu] * 0x01010101u;
      o = make_uint4(r, r, r, r);
    } else {
      o = make_uint4(map4(w.x, lut), map4(w.y, lut), map4(w.z, lut), map4(w.w, lut));
    }
    *(uint4*)(d + p) = o;
  }
  if (blockIdx.x == 0) {
    if (t < head) d[t] = lut[s[t]];
    else if (t >= 16 && t - 16 < tail) d[tail_begin + t - 16] = lut[s[tail_begin + t - 16]];
  }
}
}  // namespace

extern "C" int rmem_label_census(const unsigned char* labels, int n, int H, int W, int* out, void* stream) {
  RMEM_REQUIRE(labels && out, "rmem_label_census: null pointer (labels and out are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_census: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_census: H and W must be positive, H * W at most 2^26");
  const int HW = H * W, entries = n * 256;
  hipLaunchKernelGGL(k_census_init, dim3((entries + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, out, entries, H, W);
  hipLaunchKernelGGL(k_census, dim3(blocks_per_frame(HW, n), n), dim3(kThreads), 0, (hipStream_t)stream, labels, HW, W, out);
  return rmem_check_launch("rmem_label_census");
}

extern "C" int rmem_label_remap(const unsigned char* src, unsigned char* dst, int n, long long pixels, const unsigned char* luts,
                                int lut_per_frame, void* stream) {
  RMEM_REQUIRE(src && dst && luts, "rmem_label_remap: null pointer (src, dst and luts are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_remap: n must be in 1..65535");
  RMEM_REQUIRE(pixels >= 1 && pixels <= kMaxPixels, "rmem_label_remap: pixels must be in 1..2^26");
  hipLaunchKernelGGL(k_remap, dim3(blocks_per_frame((long)pixels, n), n), dim3(kThreads), 0, (hipStream_t)stream, src, dst, (int)pixels,
                     luts, lut_per_frame);
  return rmem_check_launch("rmem_label_remap");
}
