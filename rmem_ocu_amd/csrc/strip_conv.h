// What the strip kernels of the encoder's ResNet front end share (conv3x3_direct.hip, bneck_block.hip, stem.hip): a workgroup owns
// a strip of columns and walks DOWN a run of rows, input rows go to a ring of LDS row slots once, the weights live in registers as
// the A operand.  Here: the layout of a ring row slot, the pipelined 3x3 tap loop over three such slots, and the host's partition
// of a strip into runs of rows.  Helpers only: no kernel lives here.
#pragma once
#include "common.h"
#include "lds_dma.h"

namespace {

// Byte offset of the 16-byte piece (column col, channel chunk) in a ring row slot of KC chunks per pixel.  A slot is laid out
// [column block of 16][channel chunk][column in block] x 16 B: the 16 lanes of a ds_read_b128 group read 16 CONSECUTIVE columns
// (whatever the tap shift, whatever the chunk), which then fall on 16 distinct 16-byte bank slots -- no conflicts at any alignment
// (the GEMM panels' XOR swizzle, swz(), is conflict-free only for aligned column groups: 41 % of conv3x3_direct's LDS cycles were
// conflicts with it).  Every writer and reader of a ring slot uses this one formula.  The next chunk of a pixel is 256 bytes
// further on and its next channel slice (32 channels = 4 chunks) 1024, whatever KC.
template <int KC>
__host__ __device__ __forceinline__ constexpr int ring_slot_off(int col, int chunk) { return (((col >> 4) * KC + chunk) * 16 + (col & 15)) * 16; }
// ... and its inverse: the piece at byte 16 q of a slot.  LDS-DMA fills a slot linearly, so a kernel that stages rows by LDS-DMA
// applies the layout to the SOURCE: its piece q comes from column ring_slot_col(q), chunk ring_slot_chunk(q).
template <int KC>
__host__ __device__ __forceinline__ constexpr int ring_slot_col(int q) { return (q / (16 * KC)) * 16 + (q & 15); }
template <int KC>
__host__ __device__ __forceinline__ constexpr int ring_slot_chunk(int q) { return (q >> 4) % KC; }
template <int KC>
constexpr bool ring_slot_round_trip() {
  for (int q = 0; q < 64 * KC; ++q)
    if (ring_slot_off<KC>(ring_slot_col<KC>(q), ring_slot_chunk<KC>(q)) != 16 * q) return false;
  return true;
}
static_assert(ring_slot_round_trip<8>() && ring_slot_round_trip<16>(), "ring_slot_col / ring_slot_chunk invert ring_slot_off");
static_assert(ring_slot_off<8>(0, 1) == 256 && ring_slot_off<16>(0, 4) == 1024, "chunk and channel-slice strides of a slot");

// The 3x3 over three ring row slots rb[dy] (rows y - 1 .. y + 1), weights wf in registers as the A operand: KS = 9 SPT k-slices
// of 32, tap-major, then input channel (the GEMM's k order); coff[pt][dx] = ring_slot_off of this lane's (pixel of tile pt, chunk
// lane >> 4) under horizontal tap dx.  Software-pipelined: the B fragments of slice k + 1 are requested before the MFMAs of slice k
// (at two waves per SIMD an exposed LDS round trip per slice is most of the tile otherwise).
template <int CT, int PT, int SPT>
__device__ __forceinline__ void ring3x3_mfma(const e16x8 (&wf)[CT][9 * SPT], const char* const (&rb)[3], const int (&coff)[PT][3], f32x4 (&acc)[CT][PT]) {
  constexpr int KS = 9 * SPT;
  e16x8 bf[2][PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) bf[0][pt] = *reinterpret_cast<const e16x8*>(rb[0] + coff[pt][0]);
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    if (k + 1 < KS) {
      const int tap = (k + 1) / SPT, s = (k + 1) % SPT, dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) bf[(k + 1) & 1][pt] = *reinterpret_cast<const e16x8*>(rb[dy] + coff[pt][dx] + s * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = RMEM_MFMA_16x16x32(wf[ct][k], bf[k & 1][pt], acc[ct][pt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Runs of rows per column strip (host): enough runs that `strips` strips make about target_wgs workgroups, rows per run as long as
// that allows (every run re-reads or recomputes its halo rows and re-loads the weights); forced > 0 sets the rows per run instead.
// Outputs do not depend on the partition, only the time does.
struct StripRuns {
  int nruns, run_len;
};
constexpr StripRuns strip_runs(int target_wgs, long strips, int rows, int forced = 0) {
  long nruns = (target_wgs + strips - 1) / strips;
  if (nruns < 1) nruns = 1;
  if (nruns > rows) nruns = rows;
  int run_len = (int)((rows + nruns - 1) / nruns);
  if (forced > 0) run_len = forced < rows ? forced : rows;
  return {(rows + run_len - 1) / run_len, run_len};
}
constexpr bool strip_runs_are(StripRuns r, int nruns, int run_len) { return r.nruns == nruns && r.run_len == run_len; }
static_assert(strip_runs_are(strip_runs(512, 16 * 4, 121), 8, 16), "conv3x3_direct, C = 64: 16 frames of 121 x 213");
static_assert(strip_runs_are(strip_runs(256, 16 * 4, 121), 4, 31), "bneck_block: the same frames");
static_assert(strip_runs_are(strip_runs(256, 16 * 2, 61), 8, 8), "conv3x3_direct, C = 128: 16 frames of 61 x 107");
static_assert(strip_runs_are(strip_runs(256, 1000, 10), 1, 10), "more strips than workgroups wanted: one run");
static_assert(strip_runs_are(strip_runs(512, 1, 3), 3, 1), "no more runs than rows");
static_assert(strip_runs_are(strip_runs(256, 4, 5, 2), 3, 2), "forced rows per run");
static_assert(strip_runs_are(strip_runs(256, 4, 5, 9), 1, 5), "forced rows per run, clamped to the rows there are");

}  // namespace
