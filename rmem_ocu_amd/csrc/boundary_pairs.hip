// Pair boundary census (include/rmem.h, rmem_pair_boundary_*): per frame the boundary match counts of EVERY object of stack a with
// every object of stack b -- the counts behind the DAVIS boundary accuracy F of every (predicted, annotated) pair, where
// boundary.hip compares id i with id i only and stops at 31 ids.  Up to 255 ids per side.  uint8 in, int32 out: built once.
//
// Bit planes as in boundary.hip (one 64-bit word = 64 consecutive pixels of a row), per frame of a pass
//     [num_a planes of a's ids][num_b planes of b's ids][any_a][any_b]      each [H][ceil(W/64)] words,
// any_x = the OR of all of that side's boundary words.  A pass's planes are cleared on the stream and only non-zero words are
// stored, so what the workspace held before never shows.
//   k_pplanes  one wave per word.  A lane holds its pixel's value and those of its east, south and south-east neighbours under
//              seg2bmap's edge rules, per side, void (a value of b) cleared on both sides; values that are no object become 0.
//              The ids present in the word are not collected in a 256-bit set: the wave walks the distinct values its lanes still
//              hold (label_pairs.hip's step) -- the value of the first lane with one left, one ballot of the seg2bmap predicate,
//              every lane drops that value -- and a lane whose four values are equal holds none, so a word inside an object or
//              the background costs no step at all and a word crossed by two objects costs two.  Lane 0 stores the word and adds
//              its popcount to the workgroup's LDS counter of that id; the counters go to bnd_a / bnd_b with one global add per
//              non-zero counter and workgroup.
//   k_pmatch   one workgroup per (frame, id k of the dilated side, 16 rows x 16 words), launched once per side.  It leaves at once
//              when id k has no boundary on the frame, stages k's rows y0 - r .. y1 + r (one halo word left and right) in LDS,
//              leaves when they are all zero, and dilates ONCE: each thread the centre word of its (row, word) with
//              bitplane_dilate.h's recurrence, only where the opposite side's any word is non-zero.  Then the ids of the opposite
//              side with a boundary on the frame: their own word, a ballot (skip when no lane hits), the wave's popcount sum, one
//              LDS add per wave and id, one global add per workgroup and id.
// Integer adds only: the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "common.h"
#include "bitplane_dilate.h"
#include "../../include/rmem.h"

namespace {

constexpr int kMaxIds = 255;

// One side's step for one word: c / e / s / se are the lane's four values (0 = no object).  base: the side's id planes of the
// frame, anyp: its any plane, u: the word's index in a plane, sh[k]: the workgroup's boundary count of id k.  Whole waves only.
__device__ __forceinline__ void side_words(int c, int e, int s, int se, uint64_t* __restrict__ base, uint64_t* __restrict__ anyp,
                                           long plane, int u, int lane, unsigned int* sh) {
  unsigned rem = (c == e && c == s && c == se) ? 0u : (unsigned)(c != 0) | (unsigned)(e != 0) << 1 | (unsigned)(s != 0) << 2 |
                                                          (unsigned)(se != 0) << 3;
  uint64_t any = 0;
  for (;;) {
    const uint64_t busy = __ballot(rem != 0);
    if (!busy) break;
    const int cand = (rem & 1u) ? c : (rem & 2u) ? e : (rem & 4u) ? s : se;
    const int k = __builtin_amdgcn_readlane(cand, __builtin_ctzll(busy));
    const bool qc = c == k, qe = e == k, qs = s == k, qse = se == k;
    const uint64_t w = __ballot((qc || qe || qs || qse) && !(qc && qe && qs && qse));   // never empty: the picked lane is in it
    rem &= ~((unsigned)qc | (unsigned)qe << 1 | (unsigned)qs << 2 | (unsigned)qse << 3);
    any |= w;
    if (lane == 0) {
      base[(long)(k - 1) * plane + u] = w;
      atomicAdd(&sh[k], (unsigned)__popcll(w));
    }
  }
  if (lane == 0 && any) anyp[u] = any;
}

__device__ __forceinline__ int object_of(int v, int num) { return v <= num ? v : 0; }

__global__ __launch_bounds__(256) void k_pplanes(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W, int Wq,
                                                 int num_a, int num_b, int void_label, uint64_t* __restrict__ planes,
                                                 int* __restrict__ bnd_a, int* __restrict__ bnd_b) {
  __shared__ unsigned int sh[2][kMaxIds + 1];      // per side and id: boundary pixels seen by this workgroup
  for (int i = threadIdx.x; i <= kMaxIds; i += 256) sh[0][i] = sh[1][i] = 0;
  __syncthreads();
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const long frame = (long)f * H * W;
  const long plane = (long)H * Wq;
  uint64_t* const base_a = planes + (long)f * (num_a + num_b + 2) * plane;
  uint64_t* const base_b = base_a + (long)num_a * plane;
  uint64_t* const any_a = base_b + (long)num_b * plane;
  uint64_t* const any_b = any_a + plane;
  const int units = H * Wq;
  for (int u = blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += gridDim.x * 4) {
    const int y = u / Wq, wx = u - y * Wq;
    const int x = wx * 64 + lane;
    const bool in = x < W, east = x + 1 < W, south = y + 1 < H;
    const long i = frame + (long)y * W + x;
    // the four pixels of the lane, 0 where there is none or b is void there
    int ac = 0, ae = 0, as = 0, ase = 0, bc = 0, be = 0, bs = 0, bse = 0;
    if (in) { bc = b[i]; ac = bc == void_label ? 0 : a[i]; if (bc == void_label) bc = 0; }
    if (east) { be = b[i + 1]; ae = be == void_label ? 0 : a[i + 1]; if (be == void_label) be = 0; }
    if (in && south) { bs = b[i + W]; as = bs == void_label ? 0 : a[i + W]; if (bs == void_label) bs = 0; }
    if (east && south) { bse = b[i + W + 1]; ase = bse == void_label ? 0 : a[i + W + 1]; if (bse == void_label) bse = 0; }
    // seg2bmap's edge rules: the last column compares with the south neighbour only, the last row with the east one only, the
    // bottom-right pixel with none.  A neighbour that is left out takes the centre's value, which compares equal.
    if (!east) { ae = ac; be = bc; }
    if (!south) { as = ac; bs = bc; }
    if (!east || !south) { ase = ac; bse = bc; }
    side_words(object_of(ac, num_a), object_of(ae, num_a), object_of(as, num_a), object_of(ase, num_a), base_a, any_a, plane, u, lane,
               sh[0]);
    side_words(object_of(bc, num_b), object_of(be, num_b), object_of(bs, num_b), object_of(bse, num_b), base_b, any_b, plane, u, lane,
               sh[1]);
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= kMaxIds; k += 256) {
    if (k <= num_a && sh[0][k]) atomicAdd(&bnd_a[(long)f * (num_a + 1) + k], (int)sh[0][k]);
    if (k <= num_b && sh[1][k]) atomicAdd(&bnd_b[(long)f * (num_b + 1) + k], (int)sh[1][k]);
  }
}

// kDilateB: b's id k is dilated and matched by a's boundaries (match[..][0]); otherwise a's id k by b's boundaries (match[..][1]).
template <bool kDilateB>
__global__ __launch_bounds__(256) void k_pmatch(const uint64_t* __restrict__ planes, int H, int Wq, int num_a, int num_b, int radius,
                                                int xtiles, const int* __restrict__ bnd_a, const int* __restrict__ bnd_b,
                                                int* __restrict__ match) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];      // [kRows + 2 * radius][kLdsWords]: id k's rows
  __shared__ unsigned int tot[kMaxIds + 1];                           // per opposite id: this workgroup's matches
  const int f = blockIdx.z, k = blockIdx.y + 1;
  const int* const bnd_d = kDilateB ? bnd_b + (long)f * (num_b + 1) : bnd_a + (long)f * (num_a + 1);
  const int* const bnd_o = kDilateB ? bnd_a + (long)f * (num_a + 1) : bnd_b + (long)f * (num_b + 1);
  if (bnd_d[k] == 0) return;                        // k_pplanes has finished: no boundary, nothing to dilate
  const int num_o = kDilateB ? num_a : num_b;
  const int ytile = blockIdx.x / xtiles, xtile = blockIdx.x - ytile * xtiles;
  const int y0 = ytile * kRows, w0 = xtile * kWords;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, lane = threadIdx.x & 63;
  const long plane = (long)H * Wq;
  const uint64_t* const fr = planes + (long)f * (num_a + num_b + 2) * plane;
  const uint64_t* const src = fr + (long)((kDilateB ? num_a : 0) + k - 1) * plane;
  const uint64_t* const opp = fr + (long)(kDilateB ? 0 : num_a) * plane;
  const uint64_t* const any_o = fr + (long)(num_a + num_b + (kDilateB ? 0 : 1)) * plane;
  tot[threadIdx.x] = 0;
  const int nrows = kRows + 2 * radius;
  int seen = 0;
  for (int i = threadIdx.x; i < nrows * kLdsWords; i += 256) {
    const int ry = i / kLdsWords, rx = i - ry * kLdsWords;
    const int y = y0 - radius + ry, w = w0 - 1 + rx;
    const uint64_t v = (y >= 0 && y < H && w >= 0 && w < Wq) ? src[(long)y * Wq + w] : 0;
    lds[i] = v;
    seen |= v != 0;
  }
  if (!__syncthreads_or(seen)) return;              // id k's boundary does not reach this tile
  const bool mine = y0 + ty < H && w0 + tx < Wq;
  const long at = (long)(y0 + ty) * Wq + w0 + tx;
  uint64_t D = 0;
  if (mine && any_o[at]) D = dilated_word(lds, ty, tx, radius);
  if (__ballot(D != 0)) {
    for (int j = 1; j <= num_o; ++j) {
      if (bnd_o[j] == 0) continue;
      const uint64_t hit = D ? opp[(long)(j - 1) * plane + at] & D : 0;
      if (!__ballot(hit != 0)) continue;
      int m = __popcll(hit);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
      if (lane == 0) atomicAdd(&tot[j], (unsigned)m);
    }
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j >= 1 && j <= num_o && tot[j]) {
    const int ia = kDilateB ? j : k, ib = kDilateB ? k : j;
    atomicAdd(&match[(((long)f * (num_a + 1) + ia) * (num_b + 1) + ib) * 2 + (kDilateB ? 0 : 1)], (int)tot[j]);
  }
}

inline int words_per_row(int W) { return (W + 63) / 64; }

inline bool geometry_ok(int frames, int H, int W, int num_a, int num_b) {
  return frames > 0 && frames < 65536 && H > 0 && W > 0 && (long)H * W <= (1L << 26) && (long)H * words_per_row(W) < (1L << 30) &&
         num_a >= 1 && num_a <= kMaxIds && num_b >= 1 && num_b <= kMaxIds;
}

inline size_t frame_bytes(int H, int W, int num_a, int num_b) {
  return (size_t)(num_a + num_b + 2) * (size_t)H * (size_t)words_per_row(W) * sizeof(uint64_t);
}

}  // namespace

extern "C" size_t rmem_pair_boundary_workspace_bytes(int frames, int H, int W, int num_a, int num_b) {
  if (!geometry_ok(frames, H, W, num_a, num_b)) return 0;
  return (size_t)frames * frame_bytes(H, W, num_a, num_b);
}

extern "C" int rmem_pair_boundary_counts(const unsigned char* a, const unsigned char* b, int frames, int H, int W, int num_a, int num_b,
                                         int void_label, int radius, void* workspace, size_t workspace_bytes, int* bnd_a, int* bnd_b,
                                         int* match, void* stream) {
  RMEM_REQUIRE(a && b && workspace && bnd_a && bnd_b && match, "rmem_pair_boundary_counts: null pointer");
  RMEM_REQUIRE(num_a >= 1 && num_a <= kMaxIds && num_b >= 1 && num_b <= kMaxIds,
               "rmem_pair_boundary_counts: num_a and num_b must be in 1..255");
  RMEM_REQUIRE(radius >= 1 && radius <= 63,
               "rmem_pair_boundary_counts: radius must be in 1..63 (a dilated word reaches one word to each side)");
  RMEM_REQUIRE(frames > 0 && frames < 65536, "rmem_pair_boundary_counts: frames must be in 1..65535");
  RMEM_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 26) && (long)H * words_per_row(W) < (1L << 30),
               "rmem_pair_boundary_counts: H and W must be positive, H * W at most 2^26 and H * ceil(W / 64) below 2^30");
  RMEM_REQUIRE(void_label < 0 || void_label > 255 || void_label > num_b,
               "rmem_pair_boundary_counts: a void_label inside 0..255 must lie above num_b");
  const size_t per_frame = frame_bytes(H, W, num_a, num_b);
  RMEM_REQUIRE(workspace_bytes >= per_frame, "rmem_pair_boundary_counts: the workspace is smaller than one frame's planes");
  RMEM_REQUIRE(((uintptr_t)workspace & 7u) == 0, "rmem_pair_boundary_counts: the workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t na1 = (size_t)num_a + 1, nb1 = (size_t)num_b + 1;
  if (hipMemsetAsync(bnd_a, 0, (size_t)frames * na1 * sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(bnd_b, 0, (size_t)frames * nb1 * sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(match, 0, (size_t)frames * na1 * nb1 * 2 * sizeof(int), st) != hipSuccess) {
    (void)hipGetLastError();
    rmem_set_error("rmem_pair_boundary_counts: the memset of the outputs failed");
    return -1;
  }
  const int Wq = words_per_row(W);
  const int units = H * Wq;
  const int per_frame_blocks = std::min((units + 31) / 32, 4096);   // a wave takes about 8 words, so the LDS counters are flushed rarely
  const int xtiles = (Wq + kWords - 1) / kWords, ytiles = (H + kRows - 1) / kRows;
  const size_t lds = (size_t)(kRows + 2 * radius) * kLdsWords * sizeof(uint64_t);       // 20,448 bytes at radius 63
  const int per_pass = (int)std::min<size_t>((size_t)frames, workspace_bytes / per_frame);
  for (int f0 = 0; f0 < frames; f0 += per_pass) {
    const int n = std::min(per_pass, frames - f0);
    if (hipMemsetAsync(workspace, 0, (size_t)n * per_frame, st) != hipSuccess) {
      (void)hipGetLastError();
      rmem_set_error("rmem_pair_boundary_counts: the memset of the planes failed");
      return -1;
    }
    const unsigned char* const pa = a + (size_t)f0 * H * W;
    const unsigned char* const pb = b + (size_t)f0 * H * W;
    int* const ba = bnd_a + (size_t)f0 * na1;
    int* const bb = bnd_b + (size_t)f0 * nb1;
    int* const mt = match + (size_t)f0 * na1 * nb1 * 2;
    hipLaunchKernelGGL(k_pplanes, dim3(per_frame_blocks, n), dim3(256), 0, st, pa, pb, H, W, Wq, num_a, num_b, void_label,
                       (uint64_t*)workspace, ba, bb);
    if (int rc = rmem_check_launch("rmem_pair_boundary_counts (planes)")) return rc;
    hipLaunchKernelGGL(k_pmatch<true>, dim3(xtiles * ytiles, num_b, n), dim3(256), lds, st, (const uint64_t*)workspace, H, Wq, num_a,
                       num_b, radius, xtiles, (const int*)ba, (const int*)bb, mt);
    if (int rc = rmem_check_launch("rmem_pair_boundary_counts (match a in b)")) return rc;
    hipLaunchKernelGGL(k_pmatch<false>, dim3(xtiles * ytiles, num_a, n), dim3(256), lds, st, (const uint64_t*)workspace, H, Wq, num_a,
                       num_b, radius, xtiles, (const int*)ba, (const int*)bb, mt);
    if (int rc = rmem_check_launch("rmem_pair_boundary_counts (match b in a)")) return rc;
  }
  return 0;
}
