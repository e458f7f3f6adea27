// Baseline JPEG decode on the GPU (include/rmem.h, rmem_jpeg_*): Huffman entropy decode with self-synchronisation, libjpeg's
// ISLOW IDCT, libjpeg-turbo's fancy upsampling and YCbCr->RGB, bit-exact with libjpeg-turbo (Pillow).  The packed input comes
// from rmem_jpeg_pack (jpeg_host.cpp).
//
// Entropy decode (Weissenberger & Schmidt, ICPP 2018 / HiPC 2021).  A unit (restart interval, or the whole scan) is cut into
// subsequences of RMEM_JPEG_SUBSEQ_BITS; one lane owns one.  A decoder state is (bit position p, block c inside the MCU,
// zig-zag index k); a lane decodes from its start state until the first symbol boundary at or past its end and records the
// exit state and the blocks it completed.  Phases, each a launch ordered by the stream (no communication between workgroups
// inside a launch):
//   (a) k_jpeg_sync_local   every lane decodes speculatively from (start, 0, 0); inside the workgroup a lane re-decodes from
//                           its predecessor's exit until nothing changes (the chain is anchored at the unit's first lane);
//   (b) k_jpeg_sync_global  bounded rounds of the same across workgroups; a round returns at once when the previous one
//                           changed nothing (a device counter per round);
//       k_jpeg_mark / k_jpeg_fallback   a unit whose chain is still inconsistent is decoded by one lane sequentially;
//   (c) k_jpeg_scan         segmented exclusive scan of completed blocks -> first block of every subsequence;
//   (d) k_jpeg_decode       the final decode writes int16 coefficients in natural order (DC as differences);
//   (e) k_jpeg_dc_*         segmented prefix sum of the DC differences per component, reset at each unit.
// Speculative decoding meets invalid codes by design: in the sync phases an invalid code (or coefficient index past 63) restarts
// the lane's speculation one bit further on, so a lane keeps hunting for the real symbol boundaries instead of handing a dead
// state down the chain; the final decode, which starts from real states only, reports it in the status word.  Every read
// stays inside the frame's chunk (reads past the entropy bytes see its zero padding).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "common.h"
#include "../../include/rmem.h"

namespace {

constexpr int kSub = RMEM_JPEG_SUBSEQ_BITS;
constexpr int kLanes = 64;            // lanes per workgroup of the sync / decode kernels (one wavefront)
constexpr uint64_t kDead = ~0ull;
constexpr int kMisc = 16;             // ints at off_misc: [0] units finished, [1] status bits

__constant__ unsigned char kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                           12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                           58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Slot {
  uint64_t* in;       // start state of each subsequence
  uint64_t* ex;       // exit state
  uint32_t* cnt;      // blocks completed
  uint32_t* start;    // first block (phase c)
  uint32_t* bad;      // per unit: chain inconsistent after the sync rounds
  int* dcs;           // DC scan inside a tile [max_blocks], then tile aggregates and carries
  int16_t* coef;
  unsigned char* plane;
  int* misc;
};

__host__ __device__ inline int dc_tiles(int blocks) { return (blocks + 255) / 256; }

__device__ inline Slot slot_of(void* ws, const rmem_jpeg_plan& P, int i) {
  char* b = (char*)ws + (long long)i * P.slot_bytes;
  Slot s;
  s.in = (uint64_t*)(b + P.off_state);
  s.ex = s.in + P.max_sub;
  s.cnt = (uint32_t*)(s.ex + P.max_sub);
  s.start = s.cnt + P.max_sub;
  s.bad = (uint32_t*)(b + P.off_unit);
  s.dcs = (int*)(b + P.off_dc);
  s.coef = (int16_t*)(b + P.off_coef);
  s.plane = (unsigned char*)(b + P.off_plane);
  s.misc = (int*)(b + P.off_misc);
  return s;
}

__device__ inline int* round_counters(void* ws, const rmem_jpeg_plan& P) { return (int*)((char*)ws + (long long)P.batch * P.slot_bytes); }

__host__ __device__ inline bool fits(const rmem_jpeg_desc& D, const rmem_jpeg_plan& P) {
  return D.nsub <= P.max_sub && D.total_blocks <= P.max_blocks && D.nunits <= P.max_units && D.width <= P.max_width &&
         D.height <= P.max_height && D.nsub > 0 && D.bpm >= 1 && D.bpm <= 10 && D.ncomp >= 1 && D.ncomp <= 3;
}

// the frame's entropy bytes as big-endian 32-bit words; nw covers the bytes and the chunk's zero padding
struct Bits {
  const uint32_t* w;
  uint32_t nw;
  const uint32_t* units;   // {bit offset, first subsequence} x (nunits + 1)
};

__device__ inline Bits bits_of(const unsigned char* clip, const rmem_jpeg_desc& D) {
  Bits b;
  b.units = (const uint32_t*)(clip + D.offset);
  b.w = (const uint32_t*)(clip + D.offset + D.data_off);
  b.nw = (uint32_t)(((long long)D.data_bits + 256) >> 5);
  return b;
}

__device__ inline uint32_t peek32(const Bits& b, uint32_t p) {
  const uint32_t i = p >> 5, sh = p & 31;
  const uint32_t a = i < b.nw ? __builtin_bswap32(b.w[i]) : 0u;
  const uint32_t c = i + 1 < b.nw ? __builtin_bswap32(b.w[i + 1]) : 0u;
  return sh ? (a << sh) | (c >> (32 - sh)) : a;
}

// unit of subsequence s: the last u with first_sub(u) <= s
__device__ inline int unit_of(const Bits& b, int nunits, int s) {
  int lo = 0, hi = nunits - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)b.units[2 * mid + 1] <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct SubRange {
  int unit, head;
  uint32_t begin, end;
};

__device__ inline SubRange sub_range(const Bits& b, const rmem_jpeg_desc& D, int s) {
  SubRange r;
  r.unit = unit_of(b, D.nunits, s);
  const uint32_t ub = b.units[2 * r.unit], ue = b.units[2 * r.unit + 2], fs = b.units[2 * r.unit + 1];
  r.head = (uint32_t)s == fs;
  r.begin = ub + (uint32_t)(s - (int)fs) * kSub;
  r.end = min(r.begin + (uint32_t)kSub, ue);
  return r;
}

__device__ inline uint64_t mkstate(uint32_t p, int c, int k) { return (uint64_t)p | ((uint64_t)c << 32) | ((uint64_t)k << 40); }

__device__ inline int huff(const rmem_jpeg_huff& h, uint32_t win, int& len) {
  const uint32_t e = h.lut[win >> 23];
  if (e) {
    len = (int)(e >> 8);
    return (int)(e & 255);
  }
  for (int l = 10; l <= 16; l++) {
    const int code = (int)(win >> (32 - l));
    if (code <= h.maxcode[l]) {
      len = l;
      return h.vals[(h.valoff[l] + code) & 255];
    }
  }
  return -1;
}

__device__ inline int extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// block B of the decode order (MCU B / bpm, block c of the MCU) -> its slot in the [total_blocks][64] coefficient buffer
__device__ inline int block_index(const rmem_jpeg_desc& D, int B, int c) {
  const int mcu = B / D.bpm, comp = D.mcu_comp[c], sub = D.mcu_sub[c], h = D.comp_h[comp];
  const int row = (mcu / D.mcus_x) * D.comp_v[comp] + sub / h, col = (mcu % D.mcus_x) * h + sub % h;
  return D.comp_block0[comp] + row * D.comp_bw[comp] + col;
}

// Decodes from state st until the first symbol boundary >= end.  WRITE: the final pass, which also stores coefficients of
// block B onwards, stops after block ue_blk - 1 and returns kDead at an invalid code; otherwise an invalid code restarts the
// speculation at the next bit.  Returns the exit state.
template <bool WRITE>
__device__ uint64_t run(const rmem_jpeg_desc& D, const Bits& b, uint64_t st, uint32_t end, int& count, int16_t* coef = nullptr,
                        int B = 0, int ue_blk = 0, int* finished = nullptr) {
  count = 0;
  if (st == kDead) return kDead;
  uint32_t p = (uint32_t)st;
  int c = (int)(st >> 32) & 255, k = (int)(st >> 40) & 255;
  int16_t* blk = nullptr;
  if (WRITE) blk = coef + (long long)block_index(D, B, c) * 64;
  while (p < end) {
    const uint32_t win = peek32(b, p);
    const int comp = D.mcu_comp[c];
    int len = 0;
    if (k == 0) {
      const int s = huff(D.dc[comp], win, len);
      if (s < 0) {
        if (WRITE) return kDead;
        p++, c = 0, k = 0;
        continue;
      }
      const int v = s ? extend((win << len) >> (32 - s), s) : 0;
      if (WRITE) blk[0] = (int16_t)v;
      p += len + s;
      k = 1;
    } else {
      const int rs = huff(D.ac[comp], win, len);
      const int r = rs >> 4, s = rs & 15;
      if (rs < 0 || (s && k + r > 63) || (!s && r == 15 && k + 16 > 63)) {
        if (WRITE) return kDead;
        p++, c = 0, k = 0;
        continue;
      }
      if (s) {
        k += r;
        if (WRITE) blk[kNatural[k]] = (int16_t)extend((win << len) >> (32 - s), s);
        p += len + s;
        k++;
      } else if (r == 15) {
        k += 16;
        p += len;
      } else {
        p += len;
        k = 64;
      }
    }
    if (k >= 64) {
      count++;
      k = 0;
      c = c + 1 == D.bpm ? 0 : c + 1;
      if (WRITE) {
        if (++B == ue_blk) {
          *finished = 1;
          break;
        }
        blk = coef + (long long)block_index(D, B, c) * 64;
      }
    }
  }
  return mkstate(p, c, k);
}

// ------------------------------------------------------------------------------------------------ setup
__global__ void k_jpeg_zero(const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  Slot S = slot_of(ws, P, blockIdx.y);
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  if (tid < kMisc) S.misc[tid] = (tid == 1 && !fits(D, P)) ? RMEM_JPEG_ST_DESC : 0;
  if (blockIdx.y == 0 && tid < P.sync_rounds + 2) round_counters(ws, P)[tid] = 0;
  if (!fits(D, P)) return;
  for (int u = tid; u < D.nunits; u += nth) S.bad[u] = 0;
  int4* c4 = (int4*)S.coef;
  const long long n4 = (long long)D.total_blocks * 8;   // 64 int16 = 8 x 16 bytes
  for (long long i = tid; i < n4; i += nth) c4[i] = make_int4(0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ (a), (b) synchronisation
// One workgroup = kLanes consecutive subsequences.  Returns whether any lane re-decoded.
__device__ bool sync_block(const rmem_jpeg_desc& D, const Bits& b, const SubRange& R, bool valid, int lane, uint64_t pred0,
                           uint64_t& in, uint64_t& ex, int& cnt) {
  __shared__ uint64_t lex[kLanes];
  bool any = false;
  for (int it = 0; it <= kLanes; it++) {
    lex[lane] = ex;
    __syncthreads();
    bool changed = false;
    if (valid && !R.head) {
      const uint64_t pin = lane ? lex[lane - 1] : pred0;
      if (pin != in) {
        in = pin;
        ex = run<false>(D, b, in, R.end, cnt);
        changed = true;
      }
    }
    const bool again = __syncthreads_or(changed);
    any |= again;
    if (!again) break;
  }
  return any;
}

__global__ void __launch_bounds__(kLanes) k_jpeg_sync_local(const unsigned char* __restrict__ clip, const rmem_jpeg_desc* __restrict__ descs,
                                                             int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  if (!fits(D, P) || (int)(blockIdx.x * kLanes) >= D.nsub) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  const Bits b = bits_of(clip, D);
  const int lane = threadIdx.x, s = blockIdx.x * kLanes + lane;
  const bool valid = s < D.nsub;
  SubRange R = {0, 1, 0, 0};
  uint64_t in = kDead, ex = kDead;
  int cnt = 0;
  if (valid) {
    R = sub_range(b, D, s);
    in = mkstate(R.begin, 0, 0);
    ex = run<false>(D, b, in, R.end, cnt);
  }
  // lane 0's predecessor lives in another workgroup: it keeps its speculative start here (phase b links it)
  sync_block(D, b, R, valid && lane > 0, lane, kDead, in, ex, cnt);
  if (valid) {
    S.in[s] = in;
    S.ex[s] = ex;
    S.cnt[s] = (uint32_t)cnt;
  }
}

__global__ void __launch_bounds__(kLanes) k_jpeg_sync_global(const unsigned char* __restrict__ clip, const rmem_jpeg_desc* __restrict__ descs,
                                                              int first, rmem_jpeg_plan P, void* ws, int round, int* stats) {
  int* ctr = round_counters(ws, P);
  if (round > 0 && __hip_atomic_load(&ctr[round - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  if (stats && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(&stats[0], 1);
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  if (!fits(D, P) || (int)(blockIdx.x * kLanes) >= D.nsub) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  const Bits b = bits_of(clip, D);
  const int lane = threadIdx.x, s = blockIdx.x * kLanes + lane;
  const bool valid = s < D.nsub;
  SubRange R = {0, 1, 0, 0};
  uint64_t in = kDead, ex = kDead, pred0 = kDead;
  int cnt = 0;
  if (valid) {
    R = sub_range(b, D, s);
    in = S.in[s];
    ex = S.ex[s];
    cnt = (int)S.cnt[s];
    if (lane == 0 && !R.head) pred0 = __hip_atomic_load(&S.ex[s - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // lane 0 without a new predecessor state keeps its own (in == pred0 then holds trivially only if they agree)
  const bool lane0_link = lane != 0 || (valid && !R.head);
  const bool any = sync_block(D, b, R, valid && lane0_link, lane, pred0, in, ex, cnt);
  if (valid) {
    S.in[s] = in;
    __hip_atomic_store(&S.ex[s], ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S.cnt[s] = (uint32_t)cnt;
  }
  if (any && threadIdx.x == 0) atomicAdd(&ctr[round], 1);
}

// a unit whose chain is still inconsistent (or every unit, with RMEM_JPEG_FORCE_FALLBACK) goes to the sequential decoder
__global__ void k_jpeg_mark(const unsigned char* __restrict__ clip, const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P,
                            void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (!fits(D, P) || s >= D.nsub) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  const Bits b = bits_of(clip, D);
  const SubRange R = sub_range(b, D, s);
  if ((P.flags & RMEM_JPEG_FORCE_FALLBACK) ? R.head : (!R.head && S.in[s] != S.ex[s - 1])) S.bad[R.unit] = 1;
}

__global__ void k_jpeg_fallback(const unsigned char* __restrict__ clip, const rmem_jpeg_desc* __restrict__ descs, int first,
                                rmem_jpeg_plan P, void* ws, int* stats) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (!fits(D, P) || u >= D.nunits) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  if (!S.bad[u]) return;
  if (stats) atomicAdd(&stats[1], 1);
  const Bits b = bits_of(clip, D);
  const int s0 = (int)b.units[2 * u + 1], s1 = (int)b.units[2 * u + 3];
  uint64_t st = mkstate(b.units[2 * u], 0, 0);
  for (int s = s0; s < s1; s++) {
    const uint32_t end = min(b.units[2 * u] + (uint32_t)(s - s0 + 1) * kSub, b.units[2 * u + 2]);
    int cnt = 0;
    S.in[s] = st;
    st = run<false>(D, b, st, end, cnt);
    S.ex[s] = st;
    S.cnt[s] = (uint32_t)cnt;
  }
}

// ------------------------------------------------------------------------------------------------ (c) first block per subsequence
// start[s] = unit's first block at a unit head, else start[s - 1] + cnt[s - 1]: a segmented inclusive scan, one workgroup per frame
__global__ void __launch_bounds__(256) k_jpeg_scan(const unsigned char* __restrict__ clip, const rmem_jpeg_desc* __restrict__ descs,
                                                   int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  if (!fits(D, P)) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  const Bits b = bits_of(clip, D);
  __shared__ int fl[256], va[256];
  __shared__ int carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  const int upu = D.restart_mcus ? D.restart_mcus : D.mcus_x * D.mcus_y;   // MCUs per unit
  for (int base = 0; base < D.nsub; base += 256) {
    const int s = base + t;
    int f = 1, v = 0;
    if (s < D.nsub) {
      const int u = unit_of(b, D.nunits, s);
      f = (int)b.units[2 * u + 1] == s;
      v = f ? u * upu * D.bpm : (int)S.cnt[s - 1];
    }
    if (t == 0 && !f) v += carry;
    f |= t == 0;
    fl[t] = f;
    va[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int pf = t >= o ? fl[t - o] : 1, pv = t >= o ? va[t - o] : 0;
      __syncthreads();
      if (!f) {
        v += pv;
        f = pf;
      }
      fl[t] = f;
      va[t] = v;
      __syncthreads();
    }
    if (s < D.nsub) S.start[s] = (uint32_t)v;
    __syncthreads();
    if (t == 255) carry = v;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ (d) final decode
__global__ void __launch_bounds__(kLanes) k_jpeg_decode(const unsigned char* __restrict__ clip, const rmem_jpeg_desc* __restrict__ descs,
                                                         int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  const int s = blockIdx.x * kLanes + threadIdx.x;
  if (!fits(D, P) || s >= D.nsub) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  const Bits b = bits_of(clip, D);
  const SubRange R = sub_range(b, D, s);
  const uint64_t in = S.in[s];
  if (in == kDead) return;                       // the lane that went dead on the real chain reports it
  const int B = (int)S.start[s];
  const int mcus = D.mcus_x * D.mcus_y;
  const int ue_blk = D.restart_mcus ? min(mcus, (R.unit + 1) * D.restart_mcus) * D.bpm : mcus * D.bpm;
  if (B >= ue_blk) return;                       // only the unit's padding bits are left
  const int c = (int)(in >> 32) & 255;
  if (B < 0 || B % D.bpm != c) {
    atomicOr(&S.misc[1], RMEM_JPEG_ST_COUNT);
    return;
  }
  int cnt = 0, finished = 0;
  const uint64_t ex = run<true>(D, b, in, R.end, cnt, S.coef, B, ue_blk, &finished);
  if (ex == kDead) atomicOr(&S.misc[1], RMEM_JPEG_ST_CODE);
  if (finished) atomicAdd(&S.misc[0], 1);
}

// ------------------------------------------------------------------------------------------------ (e) DC differences -> values
// Component ordinals (decode order within one component) map to plane blocks; heads (DC predictor reset) sit at multiples of
// the unit length in ordinals.
__device__ inline int ordinal_block(const rmem_jpeg_desc& D, int c, int o) {
  const int h = D.comp_h[c], v = D.comp_v[c], hv = h * v;
  const int mcu = o / hv, w = o % hv;
  const int row = (mcu / D.mcus_x) * v + w / h, col = (mcu % D.mcus_x) * h + w % h;
  return D.comp_block0[c] + row * D.comp_bw[c] + col;
}
__device__ inline int unit_ordinals(const rmem_jpeg_desc& D, int c) {
  return D.restart_mcus ? D.restart_mcus * D.comp_h[c] * D.comp_v[c] : 0x7fffffff;
}
// tile t of the frame (tiles of all components back to back) -> component and first ordinal; false past the last tile
__device__ inline bool tile_of(const rmem_jpeg_desc& D, int t, int& c, int& o0, int& tbase) {
  tbase = 0;
  for (c = 0; c < D.ncomp; c++) {
    const int nt = dc_tiles(D.comp_bw[c] * D.comp_bh[c]);
    if (t < tbase + nt) {
      o0 = (t - tbase) * 256;
      return true;
    }
    tbase += nt;
  }
  return false;
}

__global__ void __launch_bounds__(256) k_jpeg_dc_tiles(const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  int c, o0, tb;
  if (!fits(D, P) || !tile_of(D, blockIdx.x, c, o0, tb)) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  __shared__ int fl[256], va[256];
  const int t = threadIdx.x, o = o0 + t, n = D.comp_bw[c] * D.comp_bh[c], L = unit_ordinals(D, c);
  int f = 1, v = 0;
  if (o < n) {
    v = S.coef[(long long)ordinal_block(D, c, o) * 64];
    f = o % L == 0;
  }
  for (int d = 1; d < 256; d <<= 1) {
    fl[t] = f;
    va[t] = v;
    __syncthreads();
    const int pf = t >= d ? fl[t - d] : 1, pv = t >= d ? va[t - d] : 0;
    __syncthreads();
    if (!f) {
      v += pv;
      f = pf;
    }
  }
  if (o < n) S.dcs[D.comp_block0[c] + o] = v;
  const int last = min(n, o0 + 256) - 1;
  if (o == last) S.dcs[P.max_blocks + blockIdx.x] = v;     // tile aggregate since its last head
}

// per component: carry into every tile; thread 0 also writes the frame's status word
__global__ void k_jpeg_dc_carry(const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P, void* ws, int* status) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  Slot S = slot_of(ws, P, blockIdx.y);
  const int c = threadIdx.x;
  if (!fits(D, P)) {
    if (c == 0) status[blockIdx.y] = S.misc[1] | RMEM_JPEG_ST_DESC;
    return;
  }
  if (c == 0) status[blockIdx.y] = S.misc[1] | (S.misc[0] != D.nunits ? RMEM_JPEG_ST_COUNT : 0);
  if (c >= D.ncomp) return;
  int tb = 0;
  for (int i = 0; i < c; i++) tb += dc_tiles(D.comp_bw[i] * D.comp_bh[i]);
  const int n = D.comp_bw[c] * D.comp_bh[c], nt = dc_tiles(n), L = unit_ordinals(D, c);
  int* agg = S.dcs + P.max_blocks;
  int* car = agg + dc_tiles(P.max_blocks) + 3;
  int carry = 0;
  for (int t = 0; t < nt; t++) {
    const int o0 = t * 256, o1 = min(n, o0 + 256) - 1;
    car[tb + t] = carry;
    const bool head = o1 / L * L >= o0;
    carry = head ? agg[tb + t] : carry + agg[tb + t];
  }
}

__global__ void __launch_bounds__(256) k_jpeg_dc_apply(const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  int c, o0, tb;
  if (!fits(D, P) || !tile_of(D, blockIdx.x, c, o0, tb)) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  const int o = o0 + threadIdx.x, n = D.comp_bw[c] * D.comp_bh[c], L = unit_ordinals(D, c);
  if (o >= n) return;
  const int* car = S.dcs + P.max_blocks + dc_tiles(P.max_blocks) + 3;
  int v = S.dcs[D.comp_block0[c] + o];
  if (o / L * L < o0) v += car[blockIdx.x];           // no head between the tile start and o
  S.coef[(long long)ordinal_block(D, c, o) * 64] = (int16_t)v;
}

// ------------------------------------------------------------------------------------------------ dequantise + ISLOW IDCT
// jidctint.c: CONST_BITS 13, PASS1_BITS 2, DESCALE rounding, and the post-IDCT range limit (x & 1023 through
// sample_range_limit + CENTERJSAMPLE).  Eight threads per block: one column in pass 1, one row in pass 2.
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ inline void idct8(int i0, int i1, int i2, int i3, int i4, int i5, int i6, int i7, int o[8], int shift, int bias) {
  int z2 = i2, z3 = i6;
  int z1 = (z2 + z3) * FIX_0_541196100;
  const int tmp2 = z1 + z3 * -FIX_1_847759065, tmp3 = z1 + z2 * FIX_0_765366865;
  const int t0 = (i0 + i4) * 8192 + bias, t1 = (i0 - i4) * 8192 + bias;   // LEFT_SHIFT(.., CONST_BITS) + rounding
  const int tmp10 = t0 + tmp3, tmp13 = t0 - tmp3, tmp11 = t1 + tmp2, tmp12 = t1 - tmp2;
  int a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  z2 = a1 + a2;
  z3 = a0 + a2;
  int z4 = a1 + a3;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  a0 *= FIX_0_298631336;
  a1 *= FIX_2_053119869;
  a2 *= FIX_3_072711026;
  a3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 = z3 * -FIX_1_961570560 + z5;
  z4 = z4 * -FIX_0_390180644 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  o[0] = (tmp10 + a3) >> shift;
  o[7] = (tmp10 - a3) >> shift;
  o[1] = (tmp11 + a2) >> shift;
  o[6] = (tmp11 - a2) >> shift;
  o[2] = (tmp12 + a1) >> shift;
  o[5] = (tmp12 - a1) >> shift;
  o[3] = (tmp13 + a0) >> shift;
  o[4] = (tmp13 - a0) >> shift;
}

__device__ inline unsigned idct_limit(int x) {
  x &= 1023;
  return x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896;
}

__global__ void __launch_bounds__(256) k_jpeg_idct(const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P, void* ws) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  if (!fits(D, P)) return;
  const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int blk = blockIdx.x * 32 + lb;
  __shared__ int wsp[32][64];
  Slot S = slot_of(ws, P, blockIdx.y);
  const bool valid = blk < D.total_blocks;
  int c = 0;
  if (valid) {
    while (c + 1 < D.ncomp && blk >= D.comp_block0[c + 1]) c++;
    const int16_t* cf = S.coef + (long long)blk * 64;
    const unsigned short* q = D.quant[c];
    int o[8];
    // pass 1: column j; DESCALE(x, CONST_BITS - PASS1_BITS)
    idct8(cf[j] * q[j], cf[8 + j] * q[8 + j], cf[16 + j] * q[16 + j], cf[24 + j] * q[24 + j], cf[32 + j] * q[32 + j],
          cf[40 + j] * q[40 + j], cf[48 + j] * q[48 + j], cf[56 + j] * q[56 + j], o, 11, 1 << 10);
    for (int r = 0; r < 8; r++) wsp[lb][r * 8 + j] = o[r];
  }
  __syncthreads();
  if (!valid) return;
  const int* w = wsp[lb] + j * 8;
  int o[8];
  // pass 2: row j; DESCALE(x, CONST_BITS + PASS1_BITS + 3)
  idct8(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o, 18, 1 << 17);
  uint32_t lo = 0, hi = 0;
  for (int x = 0; x < 4; x++) lo |= idct_limit(o[x]) << (8 * x);
  for (int x = 0; x < 4; x++) hi |= idct_limit(o[4 + x]) << (8 * x);
  const int local = blk - D.comp_block0[c], bw = D.comp_bw[c];
  const int brow = local / bw, bcol = local % bw;
  unsigned char* dst = S.plane + (long long)D.comp_block0[c] * 64 + ((long long)brow * 8 + j) * (bw * 8) + bcol * 8;
  *(uint2*)dst = make_uint2(lo, hi);
}

// ------------------------------------------------------------------------------------------------ upsample + colour
// libjpeg-turbo: fancy (triangle) upsampling when downsampled_width > 2, else replication; edges replicate the first / last
// row and column of the downsampled_width x downsampled_height samples.  jdcolor.c tables with SCALEBITS 16.
__device__ inline int chroma(const unsigned char* pl, int stride, int dw, int dh, int h2, int v2, int x, int y) {
  if (!h2) return pl[(long long)y * stride + x];
  if (dw <= 2) return pl[(long long)(v2 ? y >> 1 : y) * stride + (x >> 1)];
  const int j = x >> 1, jn = (x & 1) ? min(j + 1, dw - 1) : max(j - 1, 0);
  if (!v2) {
    const unsigned char* r = pl + (long long)y * stride;
    return (x & 1) ? (3 * r[j] + r[jn] + 2) >> 2 : (3 * r[j] + r[jn] + 1) >> 2;
  }
  const int i = y >> 1, in_ = (y & 1) ? min(i + 1, dh - 1) : max(i - 1, 0);
  const unsigned char* r0 = pl + (long long)i * stride;
  const unsigned char* r1 = pl + (long long)in_ * stride;
  const int cs = 3 * r0[j] + r1[j], cn = 3 * r0[jn] + r1[jn];
  return (x & 1) ? (3 * cs + cn + 7) >> 4 : (3 * cs + cn + 8) >> 4;
}

__device__ inline unsigned char clamp255(int v) { return (unsigned char)min(max(v, 0), 255); }

__global__ void __launch_bounds__(256) k_jpeg_color(const rmem_jpeg_desc* __restrict__ descs, int first, rmem_jpeg_plan P, void* ws,
                                                    unsigned char* const* __restrict__ out) {
  const rmem_jpeg_desc& D = descs[first + blockIdx.y];
  if (!fits(D, P)) return;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.z * 4 + (threadIdx.x >> 6);
  if (x >= D.width || y >= D.height) return;
  Slot S = slot_of(ws, P, blockIdx.y);
  unsigned char* o = out[blockIdx.y] + ((long long)y * D.width + x) * 3;
  const int sy = D.comp_bw[0] * 8;
  const int Y = S.plane[(long long)y * sy + x];
  if (D.ncomp == 1) {
    o[0] = o[1] = o[2] = (unsigned char)Y;
    return;
  }
  const int h2 = D.hmax == 2, v2 = D.vmax == 2;
  const int sc = D.comp_bw[1] * 8;
  const int cb = chroma(S.plane + (long long)D.comp_block0[1] * 64, sc, D.comp_dw[1], D.comp_dh[1], h2, v2, x, y) - 128;
  const int cr = chroma(S.plane + (long long)D.comp_block0[2] * 64, sc, D.comp_dw[2], D.comp_dh[2], h2, v2, x, y) - 128;
  constexpr int kHalf = 1 << 15;
  // FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414) at SCALEBITS 16
  o[0] = clamp255(Y + ((91881 * cr + kHalf) >> 16));
  o[1] = clamp255(Y + ((-46802 * cr + -22554 * cb + kHalf) >> 16));
  o[2] = clamp255(Y + ((116130 * cb + kHalf) >> 16));
}

inline int launch_ok(const char* what) { return rmem_check_launch(what); }

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" size_t rmem_jpeg_workspace_bytes(const rmem_jpeg_desc* descs, int ndesc, int batch, rmem_jpeg_plan* plan) {
  if (!descs || ndesc <= 0 || batch <= 0 || !plan) {
    rmem_set_error("rmem_jpeg_workspace_bytes: bad arguments");
    return 0;
  }
  rmem_jpeg_plan P = {};
  P.batch = batch;
  P.sync_rounds = 8;
  for (int i = 0; i < ndesc; i++) {
    const rmem_jpeg_desc& D = descs[i];
    P.max_width = std::max(P.max_width, D.width);
    P.max_height = std::max(P.max_height, D.height);
    P.max_sub = std::max(P.max_sub, D.nsub);
    P.max_blocks = std::max(P.max_blocks, D.total_blocks);
    P.max_units = std::max(P.max_units, D.nunits);
  }
  auto al = [](long long v) { return (v + 255) & ~255LL; };
  long long o = 0;
  P.off_state = o;
  o = al(o + 24LL * P.max_sub);
  P.off_unit = o;
  o = al(o + 4LL * P.max_units);
  P.off_dc = o;
  o = al(o + 4LL * (P.max_blocks + 2 * (dc_tiles(P.max_blocks) + 3)));
  P.off_coef = o;
  o = al(o + 128LL * P.max_blocks);
  P.off_plane = o;
  o = al(o + 64LL * P.max_blocks);
  P.off_misc = o;
  o = al(o + 4LL * kMisc);
  P.slot_bytes = o;
  *plan = P;
  return (size_t)(o * batch + 256);
}

static int check_plan(const rmem_jpeg_plan* P, int n, const char* who) {
  char b[256];
  if (!P || n <= 0 || n > P->batch || P->slot_bytes <= 0 || P->sync_rounds < 0 || P->sync_rounds > 60) {
    snprintf(b, sizeof(b), "%s: bad plan or frame count", who);
    rmem_set_error(b);
    return -1;
  }
  return 0;
}

extern "C" int rmem_jpeg_entropy_decode(const unsigned char* bits, const rmem_jpeg_desc* descs, int first, int n,
                                        const rmem_jpeg_plan* plan, void* workspace, int* status, int* stats, void* stream) {
  if (check_plan(plan, n, "rmem_jpeg_entropy_decode")) return -1;
  RMEM_REQUIRE(bits && descs && workspace && status && first >= 0, "rmem_jpeg_entropy_decode: null argument");
  const rmem_jpeg_plan P = *plan;
  hipStream_t st = (hipStream_t)stream;
  const int gsub = (P.max_sub + kLanes - 1) / kLanes;
  k_jpeg_zero<<<dim3(std::max(1, std::min(1024, P.max_blocks / 32 + 1)), n), 256, 0, st>>>(descs, first, P, workspace);
  k_jpeg_sync_local<<<dim3(gsub, n), kLanes, 0, st>>>(bits, descs, first, P, workspace);
  for (int r = 0; r < P.sync_rounds; r++)
    k_jpeg_sync_global<<<dim3(gsub, n), kLanes, 0, st>>>(bits, descs, first, P, workspace, r, stats);
  k_jpeg_mark<<<dim3((P.max_sub + 255) / 256, n), 256, 0, st>>>(bits, descs, first, P, workspace);
  k_jpeg_fallback<<<dim3((P.max_units + 63) / 64, n), 64, 0, st>>>(bits, descs, first, P, workspace, stats);
  k_jpeg_scan<<<dim3(1, n), 256, 0, st>>>(bits, descs, first, P, workspace);
  k_jpeg_decode<<<dim3(gsub, n), kLanes, 0, st>>>(bits, descs, first, P, workspace);
  const int tiles = dc_tiles(P.max_blocks) + 3;
  k_jpeg_dc_tiles<<<dim3(tiles, n), 256, 0, st>>>(descs, first, P, workspace);
  k_jpeg_dc_carry<<<dim3(1, n), 64, 0, st>>>(descs, first, P, workspace, status);
  k_jpeg_dc_apply<<<dim3(tiles, n), 256, 0, st>>>(descs, first, P, workspace);
  return launch_ok("rmem_jpeg_entropy_decode");
}

extern "C" int rmem_jpeg_coef_to_rgb(const rmem_jpeg_desc* descs, int first, int n, const rmem_jpeg_plan* plan, void* workspace,
                                     unsigned char* const* out, void* stream) {
  if (check_plan(plan, n, "rmem_jpeg_coef_to_rgb")) return -1;
  RMEM_REQUIRE(descs && workspace && out && first >= 0, "rmem_jpeg_coef_to_rgb: null argument");
  const rmem_jpeg_plan P = *plan;
  hipStream_t st = (hipStream_t)stream;
  k_jpeg_idct<<<dim3((P.max_blocks + 31) / 32, n), 256, 0, st>>>(descs, first, P, workspace);
  k_jpeg_color<<<dim3((P.max_width + 63) / 64, n, (P.max_height + 3) / 4), 256, 0, st>>>(descs, first, P, workspace, out);
  return launch_ok("rmem_jpeg_coef_to_rgb");
}

extern "C" int rmem_jpeg_decode_batch(const unsigned char* bits, const rmem_jpeg_desc* descs, int first, int n, const rmem_jpeg_plan* plan,
                                      void* workspace, unsigned char* const* out, int* status, int* stats, void* stream) {
  int rc = rmem_jpeg_entropy_decode(bits, descs, first, n, plan, workspace, status, stats, stream);
  if (rc) return rc;
  return rmem_jpeg_coef_to_rgb(descs, first, n, plan, workspace, out, stream);
}
