// Pair census (include/rmem.h, rmem_label_pair_census): per frame the joint histogram of (value in stack a, value in stack b) --
// the one small table behind the IoU of every predicted with every annotated object (pairs.py: pair_iou, track_iou, assign) and
// what evaluator.relabel_to_match / identity_report read.  label_census.hip's wave step, for two stacks at once.
// Element-type agnostic (uint8 in, int32 out): built once.
//
//   k_pairs    A frame is a flat range of H * W pixels in both stacks; either may start at any byte.  The walk is aligned on a:
//              single pixels up to a's first 16-byte boundary (head) and after its last one (tail), 16 pixels per lane in
//              between -- one aligned 16-byte load from a, and from b the 16 bytes at the same pixel offset, which is the same
//              aligned load when b's frame starts at a's alignment and a load of exactly those 16 bytes at their own alignment
//              otherwise (never a byte outside either stack).  A lane's 16 pixels are 16 keys (a << 8) | b.  A lane never adds a
//              pixel to the table on its own -- label maps are long runs, 64 lanes would queue on one address.  Per wave, for every
//              distinct key among the lanes' pixels (picked from the first lane that still has pixels left): each lane's 16-bit
//              mask of its pixels with that key, the wave's popcount total, one add by one lane.  A lane whose 16 pixels are one
//              pair compares one key instead of 16; a wave whose 1024 pixels are one pair needs no reduction at all.
//              Values are clamped to the "other" bins only where a key becomes a table index: two raw keys that share a bin
//              cost two adds and give the same sum.
//   routes     Tables of up to kLdsBins bins live in LDS, one per workgroup (a workgroup works on one frame), and their non-zero
//              entries are flushed with global integer adds; larger tables (up to 257 x 257) take the wave's add straight to
//              global memory.  Integer adds only: the result does not depend on the order of arrival.  out is zeroed on the
//              stream by a memset before the kernel.
#include "label_wave.h"
#include "../../include/rmem.h"

namespace {
// 32 KiB of LDS at the most: five such workgroups fit a CU's 160 KiB (the 64 KiB a workgroup gets without opting in would leave
// two), squares up to 88 + 2 fit, and a flush is at most 32 entries per thread.  The table is dynamic LDS of its own size, so a
// 12 x 12 table costs 576 bytes and leaves the occupancy to the registers.
constexpr int kLdsBins = 8192;

// the 16 bytes at p, whatever p's alignment: exactly these bytes are read
__device__ __forceinline__ uint4 load16_any(const unsigned char* p) {
  uint4 w;
  __builtin_memcpy(&w, p, 16);
  return w;
}

struct Bins {
  int num_a, num_b;
  __device__ __forceinline__ int of(int key) const {   // key = (a << 8) | b -> row min(a, num_a + 1), column min(b, num_b + 1)
    return min(key >> 8, num_a + 1) * (num_b + 2) + min(key & 0xff, num_b + 1);
  }
};

// One wave's step: lane l holds the pixels `rem` (a 16-bit mask; 0 = nothing) of wa / wb.  Called by whole waves only.  tab: the
// frame's table, in LDS (kLds) or in global memory.
template <bool kLds>
__device__ __forceinline__ void wave_pairs(uint4 wa, uint4 wb, unsigned rem, int lane, Bins bins, int* tab) {
  const bool uni = rem == 0xffffu && all_equal(wa) && all_equal(wb);
  const int first = (int)(((wa.x & 0xffu) << 8) | (wb.x & 0xffu));
  if (__ballot(uni) == ~0ull) {
    const int v = __builtin_amdgcn_readfirstlane(first);
    if (__ballot(first == v) == ~0ull) {             // the wave's 1024 pixels are one pair
      if (lane == 0) atomicAdd(tab + bins.of(v), 64 * 16);
      return;
    }
  }
  for (;;) {
    const uint64_t busy = __ballot(rem != 0);
    if (!busy) break;
    const int j = rem ? __builtin_ctz(rem) : 0;
    const int cand = (byte_at(wa, j) << 8) | byte_at(wb, j);
    const int v = __builtin_amdgcn_readlane(cand, __builtin_ctzll(busy));
    unsigned m;
    if (uni) m = first == v ? 0xffffu : 0u;          // the cheap path: one compare for 16 equal pixels
    else m = eq16(wa, v >> 8) & eq16(wb, v & 0xff) & rem;
    rem &= ~m;
    const uint64_t hit = __ballot(m != 0);           // never empty: the lane v was picked from holds it
    const int count = __ballot(m == 0xffffu) == hit ? 16 * __popcll(hit) : wave_isum(__popc(m));
    if (lane == 0) atomicAdd(tab + bins.of(v), count);
  }
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_pairs(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int HW,
                                                    int num_a, int num_b, int* __restrict__ out) {
  extern __shared__ int lds_tab[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int f = blockIdx.y;
  const Bins bins{num_a, num_b};
  const int nbins = (num_a + 2) * (num_b + 2);
  int* gtab = out + (size_t)f * nbins;
  int* tab = gtab;
  if (kLds) {
    for (int i = t; i < nbins; i += kThreads) lds_tab[i] = 0;
    __syncthreads();
    tab = lds_tab;
  }
  const unsigned char* pa = a + (size_t)f * HW;
  const unsigned char* pb = b + (size_t)f * HW;
  int head = (int)((16u - (unsigned)((uintptr_t)pa & 15u)) & 15u);
  if (head > HW) head = HW;
  const int nchunks = (HW - head) >> 4;
  const int tail_begin = head + 16 * nchunks, tail = HW - tail_begin;
  const bool b_wide = (((uintptr_t)pb + head) & 15u) == 0;      // uniform per frame
  for (int c0 = (blockIdx.x * kWaves + wave) * 64; c0 < nchunks; c0 += gridDim.x * kThreads) {
    const int c = c0 + lane;
    uint4 wa = make_uint4(0, 0, 0, 0), wb = make_uint4(0, 0, 0, 0);
    unsigned rem = 0;
    if (c < nchunks) {
      const int p = head + 16 * c;
      wa = *(const uint4*)(pa + p);
      wb = b_wide ? *(const uint4*)(pb + p) : load16_any(pb + p);
      rem = 0xffffu;
    }
    wave_pairs<kLds>(wa, wb, rem, lane, bins, tab);
  }
  if (blockIdx.x == 0 && wave == 0 && head + tail > 0) {        // lanes 0..14: the head's pixels, lanes 16..30: the tail's
    int p = -1;
    if (lane < head) p = lane;
    else if (lane >= 16 && lane - 16 < tail) p = tail_begin + lane - 16;
    uint4 wa = make_uint4(0, 0, 0, 0), wb = make_uint4(0, 0, 0, 0);
    unsigned rem = 0;
    if (p >= 0) {
      wa.x = pa[p];
      wb.x = pb[p];
      rem = 1u;
    }
    wave_pairs<kLds>(wa, wb, rem, lane, bins, tab);
  }
  if (kLds) {
    __syncthreads();
    for (int i = t; i < nbins; i += kThreads) {
      const int v = lds_tab[i];
      if (v) atomicAdd(gtab + i, v);
    }
  }
}
}  // namespace

extern "C" int rmem_label_pair_census_lds_bins(void) { return kLdsBins; }

extern "C" int rmem_label_pair_census(const unsigned char* a, const unsigned char* b, int n, int H, int W, int num_a, int num_b, int* out,
                                      void* stream) {
  RMEM_REQUIRE(a && b && out, "rmem_label_pair_census: null pointer (a, b and out are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_pair_census: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_pair_census: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(num_a >= 1 && num_a <= 255 && num_b >= 1 && num_b <= 255, "rmem_label_pair_census: num_a and num_b must be in 1..255");
  const int HW = H * W, nbins = (num_a + 2) * (num_b + 2);
  if (hipMemsetAsync(out, 0, (size_t)n * nbins * sizeof(int), (hipStream_t)stream) != hipSuccess) {
    (void)hipGetLastError();
    rmem_set_error("rmem_label_pair_census: the memset of out failed");
    return -1;
  }
  const dim3 grid(blocks_per_frame(HW, n), n);
  if (nbins <= kLdsBins)
    hipLaunchKernelGGL(k_pairs<true>, grid, dim3(kThreads), nbins * sizeof(int), (hipStream_t)stream, a, b, HW, num_a, num_b, out);
  else
    hipLaunchKernelGGL(k_pairs<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, a, b, HW, num_a, num_b, out);
  return rmem_check_launch("rmem_label_pair_census");
}
