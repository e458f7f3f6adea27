// Clip scoring on the device (include/rmem.h, rmem_clip_score_*): per (frame, object id) the four counts behind the DAVIS
// boundary accuracy F (db_eval_boundary / f_measure: seg2bmap of both masks, each boundary matched against the other one
// dilated by a disk) and the two counts behind the region similarity J (db_eval_iou), from two uint8 label stacks.
//
// Everything after the first read of the labels is done on bit planes: one 64-bit word = 64 consecutive pixels of a row.
//   k_bplanes  one wave per word.  A lane holds its pixel's label and those of its east, south and south-east neighbours
//              (void cleared on both sides); per object id present in the word, one ballot of the seg2bmap predicate per side
//              gives the boundary word, two more ballots give J's intersection and union.  Lane k keeps the words of id k and
//              writes them at the end, so every word of every plane is written in every call (absent ids as zero).
//              Planes: [frame][side][id][H][ceil(W/64)] words, side 0 = prediction, 1 = annotation.
//   k_bmatch   one workgroup per (frame, id, 16 rows x 16 words).  A disk is the union over dy of horizontal runs of half-width
//              h(dy) = floor(sqrt(r^2 - dy^2)), and h falls as |dy| grows, so with B_0 = row y and
//                  B_d = widen(B_{d-1}, h(d-1) - h(d)) | row(y - d) | row(y + d)
//              B_r is the dilated row: r one-pixel widenings and 2r row ORs per word, on a (left, centre, right) word triple
//              whose edge error creeps inwards one bit per widening and so never reaches the centre word while r <= 63.
//              matches = popcount(boundary & dilated other side); only words whose own boundary word is non-zero are dilated.
//              The other side's rows y0 - r .. y1 + r (one halo word left and right, zero outside the image) are staged in LDS.
//              A (frame, id) with an empty boundary on either side matches nothing and leaves before any plane is read.
// Counts are integers summed with atomics: the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include "common.h"
#include "bitplane_dilate.h"
#include "../../include/rmem.h"

namespace {

constexpr int kNone = 256;            // a label no id equals: void, outside the image, or a neighbour the edge rule leaves out

__device__ __forceinline__ int label_at(const uint8_t* pred, const uint8_t* gt, long i, bool ok, int void_label, int& g) {
  g = kNone;
  if (!ok) return kNone;
  const int gv = gt[i];
  if (gv == void_label) return kNone;
  g = gv;
  return pred[i];
}

__device__ __forceinline__ unsigned bit_of(int label) { return label < 32 ? 1u << label : 0u; }

__global__ __launch_bounds__(256) void k_bplanes(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int H, int W, int Wq,
                                                 int num_ids, int void_label, uint64_t* __restrict__ planes,
                                                 unsigned long long* __restrict__ counts) {
  __shared__ unsigned int sh[32][4];              // per id: n_fg, n_gt, intersection, union of this workgroup
  for (int i = threadIdx.x; i < 128; i += 256) sh[i >> 2][i & 3] = 0;
  __syncthreads();
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const long frame = (long)f * H * W;
  const long plane = (long)H * Wq;
  uint64_t* const base_p = planes + (long)f * 2 * num_ids * plane;
  uint64_t* const base_g = base_p + (long)num_ids * plane;
  const unsigned id_mask = (num_ids >= 32 ? ~0u : (1u << num_ids) - 1u) & ~1u;
  const int units = H * Wq;
  for (int u = blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += gridDim.x * 4) {
    const int y = u / Wq, wx = u - y * Wq;
    const int x = wx * 64 + lane;
    const bool in = x < W, east = x + 1 < W, south = y + 1 < H;
    const long i = frame + (long)y * W + x;
    int gc, ge, gs, gse;
    const int pc = label_at(pred, gt, i, in, void_label, gc);
    int pe = label_at(pred, gt, i + 1, east, void_label, ge);
    int ps = label_at(pred, gt, i + W, in && south, void_label, gs);
    int pse = label_at(pred, gt, i + W + 1, east && south, void_label, gse);
    // seg2bmap's edge rules: the last column compares with the south neighbour only, the last row with the east one only, the
    // bottom-right pixel with none.  A neighbour that is left out takes the centre's label, which compares equal.
    if (!east) { pe = pc; ge = gc; }
    if (!south) { ps = pc; gs = gc; }
    if (!east || !south) { pse = pc; gse = gc; }
    unsigned bits = bit_of(pc) | bit_of(pe) | bit_of(ps) | bit_of(pse) | bit_of(gc) | bit_of(ge) | bit_of(gs) | bit_of(gse);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, 64);
    unsigned present = __builtin_amdgcn_readfirstlane(bits) & id_mask;
    uint64_t mine_p = 0, mine_g = 0;
    while (present) {
      const int k = __builtin_ctz(present);
      present &= present - 1;
      const bool anyp = pc == k || pe == k || ps == k || pse == k, allp = pc == k && pe == k && ps == k && pse == k;
      const bool anyg = gc == k || ge == k || gs == k || gse == k, allg = gc == k && ge == k && gs == k && gse == k;
      const uint64_t wp = __ballot(anyp && !allp), wg = __ballot(anyg && !allg);
      const uint64_t wi = __ballot(pc == k && gc == k), wu = __ballot(pc == k || gc == k);
      if (lane == k) { mine_p = wp; mine_g = wg; }
      if (lane == 0) {
        if (wp) atomicAdd(&sh[k][0], (unsigned)__popcll(wp));
        if (wg) atomicAdd(&sh[k][1], (unsigned)__popcll(wg));
        if (wi) atomicAdd(&sh[k][2], (unsigned)__popcll(wi));
        if (wu) atomicAdd(&sh[k][3], (unsigned)__popcll(wu));
      }
    }
    if (lane >= 1 && lane < num_ids) {
      base_p[lane * plane + u] = mine_p;
      base_g[lane * plane + u] = mine_g;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * num_ids; i += 256) {
    const int k = i >> 2, c = i & 3;
    if (sh[k][c]) atomicAdd(&counts[((long)f * num_ids + k) * 6 + (c < 2 ? c : c + 2)], (unsigned long long)sh[k][c]);
  }
}

// popcount(own & dilate(other side, disk r)) for the word at tile position (ty, tx); rows = the other side's staged rows
// (the tile and the recurrence: bitplane_dilate.h)
__device__ __forceinline__ unsigned match_word(uint64_t own, const uint64_t* rows, int ty, int tx, int radius) {
  return (unsigned)__popcll(own & dilated_word(rows, ty, tx, radius));
}

__global__ __launch_bounds__(256) void k_bmatch(const uint64_t* __restrict__ planes, int H, int Wq, int num_ids, int radius, int xtiles,
                                                unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];      // [2 sides][kRows + 2 * radius][kLdsWords]
  __shared__ unsigned int tot[2];
  const int f = blockIdx.z, k = blockIdx.y + 1;
  unsigned long long* const cnt = counts + ((long)f * num_ids + k) * 6;
  if (cnt[0] == 0 || cnt[1] == 0) return;          // k_bplanes has finished: an empty boundary on either side matches nothing
  const int ytile = blockIdx.x / xtiles, xtile = blockIdx.x - ytile * xtiles;
  const int y0 = ytile * kRows, w0 = xtile * kWords;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const long plane = (long)H * Wq;
  const uint64_t* const side0 = planes + ((long)f * 2 * num_ids + k) * plane;
  const uint64_t* const side1 = side0 + (long)num_ids * plane;
  const bool mine = y0 + ty < H && w0 + tx < Wq;
  const long at = (long)(y0 + ty) * Wq + w0 + tx;
  const uint64_t own0 = mine ? side0[at] : 0, own1 = mine ? side1[at] : 0;
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  const int any0 = __syncthreads_or(own0 != 0), any1 = __syncthreads_or(own1 != 0);
  if (!any0 && !any1) return;
  const int nrows = kRows + 2 * radius;
  for (int s = 0; s < 2; ++s) {
    if (!(s ? any0 : any1)) continue;              // side s is dilated only for the other side's boundary words
    const uint64_t* const src = s ? side1 : side0;
    uint64_t* const dst = lds + s * nrows * kLdsWords;
    for (int i = threadIdx.x; i < nrows * kLdsWords; i += 256) {
      const int ry = i / kLdsWords, rx = i - ry * kLdsWords;
      const int y = y0 - radius + ry, w = w0 - 1 + rx;
      dst[i] = (y >= 0 && y < H && w >= 0 && w < Wq) ? src[(long)y * Wq + w] : 0;
    }
  }
  __syncthreads();
  unsigned m0 = 0, m1 = 0;
  if (own0) m0 = match_word(own0, lds + nrows * kLdsWords, ty, tx, radius);
  if (own1) m1 = match_word(own1, lds, ty, tx, radius);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m0 += __shfl_xor(m0, o, 64);
    m1 += __shfl_xor(m1, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (m0) atomicAdd(&tot[0], m0);
    if (m1) atomicAdd(&tot[1], m1);
  }
  __syncthreads();
  if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&cnt[2 + threadIdx.x], (unsigned long long)tot[threadIdx.x]);
}

inline int words_per_row(int W) { return (W + 63) / 64; }

}  // namespace

extern "C" size_t rmem_clip_score_workspace_bytes(int frames, int H, int W, int num_ids) {
  if (frames <= 0 || H <= 0 || W <= 0 || num_ids < 2 || num_ids > 32) return 0;
  return (size_t)frames * 2 * (size_t)num_ids * (size_t)H * (size_t)words_per_row(W) * sizeof(uint64_t);
}

extern "C" int rmem_boundary_radius(int H, int W, double bound_th) {
  if (H <= 0 || W <= 0 || !(bound_th > 0.0) || bound_th > 1e6) return -1;
  if (bound_th >= 1.0) return bound_th == floor(bound_th) ? (int)bound_th : -1;      // a pixel radius is an integer
  return (int)ceil(bound_th * sqrt((double)H * H + (double)W * W));
}

extern "C" int rmem_clip_score_counts(const unsigned char* pred, const unsigned char* gt, int frames, int H, int W, int num_ids,
                                      int void_label, int radius, void* workspace, unsigned long long* counts, void* stream) {
  RMEM_REQUIRE(num_ids >= 2 && num_ids <= 32, "rmem_clip_score_counts: num_ids must be in 2..32");
  RMEM_REQUIRE(radius >= 1 && radius <= 63, "rmem_clip_score_counts: radius must be in 1..63 (a dilated word reaches one word to each side)");
  RMEM_REQUIRE(frames > 0 && H > 0 && W > 0, "rmem_clip_score_counts: frames, H and W must be positive");
  RMEM_REQUIRE(pred && gt && workspace && counts, "rmem_clip_score_counts: null argument");
  const int Wq = words_per_row(W);
  RMEM_REQUIRE((long)H * Wq < (1L << 30) && frames < 65536, "rmem_clip_score_counts: frame too large, or more than 65535 frames");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)frames * num_ids * 6 * sizeof(unsigned long long), st) != hipSuccess) {
    rmem_set_error("rmem_clip_score_counts: hipMemsetAsync failed");
    return -1;
  }
  const int units = H * Wq;
  const int per_frame = std::min((units + 31) / 32, 4096);       // a wave takes about 8 words, so the LDS counters are flushed rarely
  hipLaunchKernelGGL(k_bplanes, dim3(per_frame, frames), dim3(256), 0, st, pred, gt, H, W, Wq, num_ids, void_label,
                     (uint64_t*)workspace, counts);
  if (int rc = rmem_check_launch("rmem_clip_score_counts (planes)")) return rc;
  const int xtiles = (Wq + kWords - 1) / kWords, ytiles = (H + kRows - 1) / kRows;
  const size_t lds = (size_t)2 * (kRows + 2 * radius) * kLdsWords * sizeof(uint64_t);      // 40,896 bytes at radius 63
  hipLaunchKernelGGL(k_bmatch, dim3(xtiles * ytiles, num_ids - 1, frames), dim3(256), lds, st, (const uint64_t*)workspace, H, Wq, num_ids,
                     radius, xtiles, counts);
  return rmem_check_launch("rmem_clip_score_counts (match)");
}
