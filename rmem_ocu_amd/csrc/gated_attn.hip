// Gated propagation attention of the DeAOT path for gfx950 (CDNA4): single head, d_att = 128, values DV = 1024 wide.
//
// Replaces layers/attention.py:138-216 (GatedPropagation.forward up to `outputs * U`; the depth-wise 5x5 and the projection
// that follow are rmem_dwconv5x5_nhwc / rmem_conv2d_nhwc calls) as called from layers/transformer.py:1183-1184 (long-term:
// keys = the restricted memory bank + temporal embedding, with the attention-weight recording of 1185-1192) and 1229
// (self-attention), and layers/attention.py:281-349 (LocalGatedPropagation: 15x15 window, learned relative embedding).
//
// With one head the value side (2 * Lq * Lk * 1024 flop) outweighs the score side (2 * Lq * Lk * 128) eight to one, and
// one 128 x Lk score matrix serves all 1024 value columns.  So, unlike the d = 32 memory read (attention.hip), the
// probabilities are materialised ONCE in e16 and the value side runs as a plain tiled GEMM:
//   k_gp_scores<., 0>  S = Q K^T (+ temporal-PE bias | window mask + relative embedding)  ->  per-chunk row maxima (sampled tiles / all)
//   k_gp_scores<., 1>  same S again (6.5 GFLOP at cfg 2, cheaper than storing fp32 S)     ->  P = exp2(S - max) in e16,
//                      [Lq][frames * Lp] with every 64-key tile fully written (zeros past a frame's end); per-chunk row sums
//   k_gp_pv            O = P V: 128 x 256 output tile per workgroup, 4 waves of 64 x 128, 64-key steps, P and V tiles
//                      through a 3-deep LDS ring filled by global_load_lds (source-side XOR swizzle), V read transposed
//                      (ds_read_b64_tr_b16); key groups give split-K slabs
//   k_gp_combine       sum the slabs, 1 / row sum, gate by U, e16 (and the per-memory-frame probability mass)
// Scores live in the log2 domain (Q pre-scaled by log2(e) / sqrt(128)).  The softmax reference is a row maximum over a SAMPLE of
// the keys (launch_all): P = 2^(S - m) keeps its 8 significant bits at every magnitude, may exceed 1, and a guard word triggers the
// exact two-pass redo (the reference is then the true row maximum, P <= 1) before fp32 could overflow.
#include "common.h"
#include "../../include/rmem.h"
#include <math.h>
#include <stdlib.h>

namespace {

constexpr int DQ = 128;    // d_att
constexpr int KT = 64;     // keys per tile
constexpr int QT = 128;    // queries per workgroup
constexpr int CW = 256;    // value columns per k_gp_pv workgroup
constexpr int MAX_ROWS = 64;
constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f;
constexpr int WIN_R = 7, WIN = 15;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ uint4 g_gp_zero16[1];

struct GpRow { int slot, kb, kn, pe_slot, t; };

struct GpParams {
  const e16* q; int ldq;
  const e16* k; long k_slot_stride; int ldk;
  const e16* v; long v_slot_stride; int ldv;
  const rmem_attn_chunk* rows; int nrows; int lk; int per;
  const float* pe_cur; const float* pe_mem;
  int Lq, Lqp;             // Lqp: Lq rounded up to QT (row count of P, mpart, lpart, slabs)
  int Lp; int ldp;         // P columns per memory frame (multiple of 64), P row stride
  float* mpart; float* lpart; e16* P;
  float qscale;
  int H, W; const float* rel; int ldrel;      // local-window mode
  int DV, nq, ncs, groups, rows_per_group;
  float* slabs;
  int debug;               // kernel experiments only (RMEM_GP_DEBUG): 1 = no MFMA, 2 = no refills after the first stages
  // softmax reference from a SAMPLE of the keys (see launch_all): sample = pass 0 visits one or two key tiles per table row only;
  // flag = launch-wide word pass 1 sets when a score exceeds the sampled reference by more than 2^64; gate = run only if *gate != 0
  int sample; unsigned* flag; const unsigned* gate;
  // several clips of identical shape in one launch: clip c's queries / one-frame keys and values / relative logits sit c * {q, k, v,
  // rel}_cs elements further (the bank is addressed through global slot indexes in the table: k_cs = v_cs = 0 there), its table
  // rows at rows + c * rows_cs, its share of the workspace c * ws_cs BYTES further
  int nclips; long q_cs, k_cs, v_cs, rel_cs, ws_cs; int rows_cs;
};

__device__ __forceinline__ void gp_select_clip(GpParams& p, int clip) {
  p.q += clip * p.q_cs; p.k += clip * p.k_cs; p.v += clip * p.v_cs;
  if (p.rows) p.rows += clip * p.rows_cs;
  if (p.rel) p.rel += clip * p.rel_cs;
  const long wf = clip * (p.ws_cs >> 2);
  p.mpart += wf; p.lpart += wf; p.slabs += wf; p.P += clip * (p.ws_cs >> 1);
}

// MODE 0: one key frame split into nrows ranges of `per` keys; 1: chunk table over the memory bank; 2: as 0 with the 15x15
// window mask and the relative embedding
template <int MODE>
__device__ __forceinline__ GpRow get_row(const GpParams& p, int r) {
  GpRow o;
  if (MODE == 1) {
    const rmem_attn_chunk c = p.rows[r];
    o.slot = c.slot; o.kb = c.key_begin; o.kn = c.key_count; o.pe_slot = c.pe_slot; o.t = c.t;
  } else {
    o.slot = 0; o.kb = r * p.per; o.kn = min(p.per, p.lk - o.kb); o.pe_slot = -1; o.t = 0;
  }
  return o;
}

__device__ __forceinline__ float half_max(float v) {      // over the 32 lanes that share lane >> 5
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// PASS 0: partial row maxima of one (query tile, table row); PASS 1: probabilities and partial row sums.
// 4 waves = (query half qh) x (key half kh): a wave owns 64 queries x 32 keys of every 64-key tile.  S = Q K^T with the
// query on the MFMA row: A = Q fragments (registers, whole kernel), B = K rows from LDS ([key][128], 16-byte chunks
// XOR-swizzled by key & 15).  The accumulator then has the KEY on the lane and 16 query rows per block in registers, so a
// row of P leaves as 32 consecutive e16.
template <int MODE, int PASS>
__global__ __launch_bounds__(256) void k_gp_scores(GpParams p) {
  __shared__ __attribute__((aligned(16))) e16 Ks[2][KT * DQ];
  __shared__ float red[2][QT];
  __shared__ float mq[QT];
  __shared__ __attribute__((aligned(16))) e16 Pst[PASS == 1 ? 4 : 1][32 * 32];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qh = wave >> 1, kh = wave & 1, lq = lane & 31, kg = lane >> 5;
  if (p.gate && *p.gate == 0) return;            // exact two-pass redo: only when the sampled reference was too low somewhere
  gp_select_clip(p, blockIdx.z);
  const int q0 = blockIdx.x * QT;
  const GpRow row = get_row<MODE>(p, blockIdx.y);
  const e16* Kp = p.k + (long)row.slot * p.k_slot_stride + (long)row.kb * p.ldk;
  const bool has_cur = MODE == 1 && p.pe_cur != nullptr;
  const bool has_mem = MODE == 1 && row.pe_slot >= 0 && p.pe_mem != nullptr;

  // ---- Q fragments (A operand): query rows 64 qh + 32 b + (lane & 31), d = 16 s + 8 kg .. + 7 ----
  e16x8 qf[2][8];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int qrow = min(q0 + 64 * qh + 32 * b + lq, p.Lq - 1);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int d0 = 16 * s + 8 * kg;
      const e16x8 raw = *reinterpret_cast<const e16x8*>(p.q + (long)qrow * p.ldq + d0);
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
      if (has_cur) { c0 = *reinterpret_cast<const f32x4*>(p.pe_cur + d0); c1 = *reinterpret_cast<const f32x4*>(p.pe_cur + d0 + 4); }
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[b][s][j] = (e16)(((float)raw[j] + (j < 4 ? c0[j & 3] : c1[j & 3])) * p.qscale);
    }
  }

  // ---- temporal-PE logit bias of this table row, per query: Qs . pe_mem[slot] through the matrix pipe.  The B operand is
  // the embedding broadcast over all 32 columns (split into e16 high + low parts: ~2^-17 relative), so every lane ends up
  // with the bias of exactly the 2 x 16 query rows its score accumulators hold ----
  f32x16 bacc[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) bacc[b][r] = 0.f;
  if (has_mem) {
    const float* pm = p.pe_mem + row.pe_slot * DQ + 8 * kg;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(pm + 16 * s), e1 = *reinterpret_cast<const f32x4*>(pm + 16 * s + 4);
      e16x8 hi8, lo8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = j < 4 ? e0[j & 3] : e1[j & 3];
        hi8[j] = (e16)e;
        lo8[j] = (e16)(e - (float)hi8[j]);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        bacc[b] = RMEM_MFMA_32x32x16(qf[b][s], hi8, bacc[b], 0, 0, 0);
        bacc[b] = RMEM_MFMA_32x32x16(qf[b][s], lo8, bacc[b], 0, 0, 0);
      }
    }
  }
  if (PASS == 1) {      // final row maximum over all table rows, via LDS
    const int ql = tid & (QT - 1), hf = tid >> 7;
    float m = NEG_BIG;
    for (int r = hf; r < p.nrows; r += 2) m = fmaxf(m, p.mpart[(long)r * p.Lqp + q0 + ql]);
    red[hf][ql] = m;
    __syncthreads();
    if (tid < QT) mq[tid] = fmaxf(red[0][tid], red[1][tid]);
    __syncthreads();
  }
  // this lane's 2 x 16 query rows: ql(b, r) = 64 qh + 32 b + (r & 3) + 8 (r >> 2) + 4 kg
  float off[2][16];      // PASS 0: bias; PASS 1: bias - row maximum
  int qyx[2][16];        // MODE 2: (qy << 16) | qx
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ql = 64 * qh + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * kg;
      off[b][r] = PASS == 1 ? bacc[b][r] - mq[ql] : bacc[b][r];
      if (MODE == 2) {
        const int qg = min(q0 + ql, p.Lq - 1);
        const int qy = qg / p.W;
        qyx[b][r] = (qy << 16) | (qg - qy * p.W);
      }
    }

  // ---- tile range: in window mode only key tiles that can intersect a window of this query tile are visited ----
  const int ntiles = (row.kn + KT - 1) / KT;
  int t_lo = 0, t_hi = ntiles;
  if (MODE == 2) {
    const int y0 = q0 / p.W, y1 = min(q0 + QT - 1, p.Lq - 1) / p.W;
    const int key_lo = max(0, (y0 - WIN_R) * p.W), key_hi = min(p.lk, (y1 + WIN_R + 1) * p.W);   // [key_lo, key_hi)
    t_lo = max(0, (key_lo - row.kb) / KT);
    t_hi = min(ntiles, (key_hi - row.kb + KT - 1) / KT);
    if (key_hi <= row.kb || key_lo >= row.kb + row.kn) { t_lo = 0; t_hi = 0; }
    if (t_hi < t_lo) t_hi = t_lo;
  }
  if (PASS == 0 && p.sample) {
    if (MODE == 2) {
      // the two key tiles that hold the query tile's OWN positions: a query's own key is always inside its window, so every
      // query gets a real score of its own as reference (rows are multiples of 64 keys and q0 of 128)
      const int s_lo = max(t_lo, (q0 - row.kb) / KT), s_hi = min(t_hi, (q0 + QT - row.kb + KT - 1) / KT);
      t_lo = q0 + QT > row.kb ? s_lo : t_hi;
      t_hi = max(t_lo, s_hi);
    } else {
      t_hi = min(t_hi, t_lo + 1);                // no mask: the first tile of the row
    }
  }
  if (p.debug & 4) t_hi = t_lo;
  e16* Pq = p.P + (long)row.t * p.Lp + row.kb;       // + q * ldp + key index inside the row
  float mx[2][16];       // PASS 0: running maxima of this lane's rows
  float gmax = NEG_BIG;                  // PASS 1: largest score above the reference this lane has seen (guard of the sampled reference)
  float ls4[4] = {0.f, 0.f, 0.f, 0.f};   // PASS 1: row-sum pieces of rows 16 i + (lane >> 2), keys 8 (lane & 3) .. + 7 of every tile
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[b][r] = NEG_BIG;
  // bias (- row maximum) as the accumulators' initial value: no per-score add
  f32x16 cinit[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) cinit[b][r] = off[b][r];

  // staging: thread -> 4 x (key, 16-byte chunk) of the 64 x 256 B tile
  e16x8 rk[4];
  const e16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto load_tile = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + 256 * i, key = id >> 4, chunk = id & 15;
      const int kidx = t * KT + key;
      rk[i] = kidx < row.kn ? *reinterpret_cast<const e16x8*>(Kp + (long)kidx * p.ldk + chunk * 8) : zero8;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + 256 * i, key = id >> 4, chunk = id & 15;
      *reinterpret_cast<e16x8*>(&Ks[buf][key * DQ + ((chunk ^ (key & 15)) << 3)]) = rk[i];
    }
  };

  if (t_lo < t_hi) {
    load_tile(t_lo);
    store_tile(0);
  }
  __syncthreads();
  const int kl = 32 * kh + lq;                        // this lane's key inside a tile
  e16* pst = &Pst[wave][0];                          // this wave's [64 q][32 keys] transposition pad
  for (int t = t_lo; t < t_hi; ++t) {
    const int cur = (t - t_lo) & 1;
    if (t + 1 < t_hi) load_tile(t + 1);
    f32x16 acc[2];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const e16x8 kf = *reinterpret_cast<const e16x8*>(&Ks[cur][kl * DQ + (((2 * s + kg) ^ (kl & 15)) << 3)]);
      acc[0] = RMEM_MFMA_32x32x16(qf[0][s], kf, s == 0 ? cinit[0] : acc[0], 0, 0, 0);
      acc[1] = RMEM_MFMA_32x32x16(qf[1][s], kf, s == 0 ? cinit[1] : acc[1], 0, 0, 0);
    }
    const int kidx = t * KT + kl;
    const bool kvalid = kidx < row.kn;
    int ky = 0, kx = 0;
    if (MODE == 2) {
      const int kgl = row.kb + kidx;
      ky = kgl / p.W;
      kx = kgl - ky * p.W;
    }
    // window mode: all 32 relative-embedding gathers of the tile are issued before any of this tile's P stores (loads and
    // stores share vmcnt, so a gather issued after a store would wait for that store to drain); the index is clamped into
    // the row so the loads are unconditional
    float rl[2][16];
    unsigned okm = 0;
    if (MODE == 2) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dy = ky - (qyx[b][r] >> 16) + WIN_R, dx = kx - (qyx[b][r] & 0xffff) + WIN_R;
          const bool in = (unsigned)dy < (unsigned)WIN && (unsigned)dx < (unsigned)WIN;
          okm |= (unsigned)in << (16 * b + r);
          const int rr = 32 * b + (r & 3) + 8 * (r >> 2) + 4 * kg;
          rl[b][r] = p.rel[(long)min(q0 + 64 * qh + rr, p.Lq - 1) * p.ldrel + (in ? dy * WIN + dx : 0)];
        }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        bool ok = kvalid;
        float sv = acc[b][r];
        const int r32 = (r & 3) + 8 * (r >> 2) + 4 * kg;             // query row inside the 32-row block b
        if (MODE == 2) {
          ok = ok && ((okm >> (16 * b + r)) & 1u);
          sv += rl[b][r] * LOG2E;
        }
        if (PASS == 0) mx[b][r] = fmaxf(mx[b][r], ok ? sv : NEG_BIG);
        else {
          pst[r32 * 32 + lq] = (e16)(ok ? __builtin_amdgcn_exp2f(sv) : 0.f);
          gmax = fmaxf(gmax, ok ? sv : NEG_BIG);
        }
      }
      if (PASS == 1) {
        // the wave's 32 x 32 block leaves as 16-byte pieces: lane -> (row 16 i + (lane >> 2), keys 8 (lane & 3) .. + 7).
        // LDS operations of one wave execute in order, so the reads see the stores above (and the next block's stores come
        // after these reads) without a barrier
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int r32 = 16 * i + (lane >> 2);
          const e16x8 v = *reinterpret_cast<const e16x8*>(&pst[r32 * 32 + (lane & 3) * 8]);
          *reinterpret_cast<e16x8*>(Pq + (long)(q0 + 64 * qh + 32 * b + r32) * p.ldp + t * KT + 32 * kh + (lane & 3) * 8) = v;
          float sum = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) sum += (float)v[j];
          ls4[2 * b + i] += sum;
        }
      }
    }
    if (t + 1 < t_hi) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- reduce over the keys (lanes) and over the two key halves (waves) ----
  if (PASS == 0) {
    // 128 rows x 64 key lanes of partial maxima through LDS (the K ring is free now): 32 dependent shuffle chains per lane
    // cost more than the whole tile loop of a short row
    float* scr = reinterpret_cast<float*>(&Ks[0][0]);            // [128 rows][64]: column 32 kh + lq
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) scr[(64 * qh + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * kg) * 64 + 32 * kh + lq] = mx[b][r];
    __syncthreads();
    {
      const int rrow = tid >> 1, hf = tid & 1;
      float m = NEG_BIG;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(&scr[rrow * 64 + 32 * hf + 4 * j]);
        m = fmaxf(fmaxf(fmaxf(m, v[0]), fmaxf(v[1], v[2])), v[3]);
      }
      m = fmaxf(m, __shfl_xor(m, 1, 64));
      if (hf == 0) { red[0][rrow] = m; red[1][rrow] = NEG_BIG; }
    }
  } else {
    // a probability above 2^64 (or a reference nobody sampled: NEG_BIG) means the sampled reference was far too low for fp32 sums:
    // ask for the exact two-pass redo (the NaN of an inf - inf would not compare, but an inf score does before it gets there)
    if (p.flag && !(gmax <= 64.f)) atomicOr(p.flag, 1u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = ls4[i];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      if ((lane & 3) == 0) red[kh][64 * qh + 16 * i + (lane >> 2)] = v;
    }
  }
  __syncthreads();
  if (tid < QT) {
    float* dst = (PASS == 0 ? p.mpart : p.lpart) + (long)blockIdx.y * p.Lqp + q0 + tid;
    if (PASS == 0) {
      const float m = fmaxf(red[0][tid], red[1][tid]);       // the bias / relative embedding is already inside every score
      *dst = m > 0.5f * NEG_BIG ? m : NEG_BIG;
    } else {
      *dst = red[0][tid] + red[1][tid];
    }
  }
}

// ---- P.V fragment plumbing (inline-asm LDS reads, counted waits) ----
struct PvFrags { e16x8 a[2]; s16x4 lo[4], hi[4]; };
constexpr int PV_PB = QT * KT * 2;            // bytes of the P tile in a stage (the V tile follows)

__device__ __forceinline__ e16x8 lds_b128(unsigned addr) {
  e16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
template <int OFF>
__device__ __forceinline__ s16x4 lds_tr16(unsigned addr) {
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
// the 10 reads of key-step S (16 keys) of the stage at LDS address sb: 2 P fragments, 4 x (low, high) V fragments
template <int S>
__device__ __forceinline__ void pv_load(unsigned sb, const int (&pa_off)[2][4], const int (&vbase)[4], PvFrags& f) {
  f.a[0] = lds_b128(sb + pa_off[0][S]);
  f.a[1] = lds_b128(sb + pa_off[1][S]);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f.lo[c] = lds_tr16<PV_PB + S * 16 * CW * 2>(sb + vbase[c]);
    f.hi[c] = lds_tr16<PV_PB + S * 16 * CW * 2 + 4 * CW * 2>(sb + vbase[c]);
  }
}
// wait until at most N LDS reads are outstanding; the fragments pass through so their consumers stay behind the wait
template <int N>
__device__ __forceinline__ void pv_wait(PvFrags& f) {
  asm volatile("s_waitcnt lgkmcnt(%10)"
               : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.lo[0]), "+v"(f.hi[0]), "+v"(f.lo[1]), "+v"(f.hi[1]), "+v"(f.lo[2]), "+v"(f.hi[2]),
                 "+v"(f.lo[3]), "+v"(f.hi[3])
               : "n"(N));
}
__device__ __forceinline__ void pv_mma(const PvFrags& f, f32x16 (&acc)[2][4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const __attribute__((ext_vector_type(8))) short b16 = {f.lo[c][0], f.lo[c][1], f.lo[c][2], f.lo[c][3],
                                                           f.hi[c][0], f.hi[c][1], f.hi[c][2], f.hi[c][3]};
    const e16x8 b = __builtin_bit_cast(e16x8, b16);
    acc[0][c] = RMEM_MFMA_32x32x16(f.a[0], b, acc[0][c], 0, 0, 0);
    acc[1][c] = RMEM_MFMA_32x32x16(f.a[1], b, acc[1][c], 0, 0, 0);
  }
}

// O = P V for one (query tile of 128, value slice of 256, key group).  Tiles of 64 keys stream through a 3-deep LDS ring
// by LDS-DMA: P tile [128 q][64 keys] (16-byte chunk c of row r at slot c ^ ((r >> 1) & 7)), V tile [64 keys][256 c]
// (chunk c of key row k at slot c ^ ((k & 3) << 2): the 32 lanes of a transposed-read half -- 4 key rows x 2 column groups
// x 4 pieces of 8 bytes -- then cover all 64 banks once).  The swizzles are applied to the per-lane SOURCE address, the LDS side of a DMA is linear.
// Waves = (query half qh) x (column half ch), 64 x 128 outputs each = 8 accumulator tiles of 32 x 32.
// PC (producer / consumer, 512 threads): waves 4..7 only issue the DMA pieces (12 per wave and tile) and count them in, waves 0..3
// only read fragments and run the MFMAs -- with one workgroup per CU the issue time of the pieces otherwise comes straight out of
// the MFMA waves' time (see gemm_conv.hip, k_conv_gemm_dma_pc).
template <int MODE, bool TIMED, bool PC = false>
__global__ __launch_bounds__(PC ? 512 : 256) void k_gp_pv(GpParams p) {
  constexpr int ST = 3, PB = QT * KT * 2, VB = KT * CW * 2, SB = PB + VB;
  __shared__ __attribute__((aligned(16))) char smem[ST * SB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = PC && wave_all >= 4;
  const int wave = PC ? (wave_all & 3) : wave_all;      // index inside the role
  const int qh = wave >> 1, ch = wave & 1, lq = lane & 31, kg = lane >> 5;
  // XCD-aware decode (hardware deals block ids round-robin over 8 XCDs): ids congruent mod 8 walk (group, query tile,
  // value slice) with the value slice fastest, so one XCD's L2 sees few distinct P and V tiles at a time
  int g, qt, cs;
  {
    const int total = p.nq * p.ncs * p.groups * p.nclips;
    const int b = blockIdx.x, xcd = b & 7, j = b >> 3;
    const int qd = total >> 3, rm = total & 7;
    const int idx = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + j;
    cs = idx % p.ncs;
    int rest = idx / p.ncs;
    qt = rest % p.nq;
    rest /= p.nq;
    g = rest % p.groups;
    gp_select_clip(p, rest / p.groups);
  }
  const int q0 = qt * QT, c0 = cs * CW;
  // table rows in LDS (scalar-like reads that do not touch vmcnt: the DMA pipeline below counts on vmcnt); the key tiles of
  // all rows form one stream that is cut into `groups` equal ranges
  __shared__ int rowtab[MAX_ROWS][4];       // slot, key_begin, key_count, P column of key 0
  __shared__ int tile_total;
  if (tid < p.nrows) {
    const GpRow r = get_row<MODE>(p, tid);
    rowtab[tid][0] = r.slot; rowtab[tid][1] = r.kb; rowtab[tid][2] = r.kn; rowtab[tid][3] = r.t * p.Lp + r.kb;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int r = 0; r < p.nrows; ++r) n += (rowtab[r][2] + KT - 1) / KT;
    tile_total = n;
  }
  __syncthreads();
  // window mode: only the key tiles that can intersect a 15x15 window of this query tile (the same band k_gp_scores<2, .>
  // visits; the probabilities outside it are never written)
  int band_lo = 0, band_hi = tile_total;
  if (p.W > 0) {
    const int y0 = q0 / p.W, y1 = min(q0 + QT - 1, p.Lq - 1) / p.W;
    band_lo = max(0, (y0 - WIN_R) * p.W) / KT;
    band_hi = min(tile_total, (min(p.lk, (y1 + WIN_R + 1) * p.W) + KT - 1) / KT);
  }
  const int tpg = (band_hi - band_lo + p.groups - 1) / p.groups;
  const int tile_begin = band_lo + g * tpg;
  const int ntl = max(0, min(band_hi, tile_begin + tpg) - tile_begin);

  // ---- DMA source bookkeeping: 4 P pieces and 8 V pieces of 16 bytes per lane and stage ----
  int p_off[4], v_key[8], v_off[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = (wave * 4 + i) * 64 + lane, r = s >> 3, lc = (s & 7) ^ ((r >> 1) & 7);
    p_off[i] = (q0 + r) * p.ldp + lc * 8;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int s = (wave * 8 + i) * 64 + lane, key = s >> 5, lc = (s & 31) ^ ((key & 3) << 2);
    v_key[i] = key;
    v_off[i] = key * p.ldv + c0 + lc * 8;
  }
  const char* zero = reinterpret_cast<const char*>(g_gp_zero16);
  // issue cursor: (row, tile inside the row) of the next tile to fetch
  int i_row = 0, i_t = tile_begin;
  while (i_row < p.nrows - 1 && i_t >= (rowtab[i_row][2] + KT - 1) / KT) { i_t -= (rowtab[i_row][2] + KT - 1) / KT; ++i_row; }
  int ir_slot = rowtab[i_row][0], ir_kb = rowtab[i_row][1], ir_kn = rowtab[i_row][2], ir_pc = rowtab[i_row][3];
  auto issue = [&](int stage) {
    char* Ps = smem + stage * SB;
    char* Vs = Ps + PB;
    const e16* psrc = p.P + ir_pc + i_t * KT;
    const e16* vsrc = p.v + (long)ir_slot * p.v_slot_stride + (long)(ir_kb + i_t * KT) * p.ldv;
    const int left = ir_kn - i_t * KT;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(psrc + p_off[i]), (lptr_t)(Ps + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const char* src = v_key[i] < left ? reinterpret_cast<const char*>(vsrc + v_off[i]) : zero;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(Vs + (wave * 8 + i) * 1024), 16, 0, 0);
    }
    if (++i_t * KT >= ir_kn) {
      i_t = 0;
      i_row = min(i_row + 1, p.nrows - 1);
      ir_slot = rowtab[i_row][0]; ir_kb = rowtab[i_row][1]; ir_kn = rowtab[i_row][2]; ir_pc = rowtab[i_row][3];
    }
  };

  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  // fragment addressing.  P (A operand): row 64 qh + 32 a + lq, logical chunk 2 s + kg.  V (B operand, transposed read):
  // the 16-lane group (lane >> 4) & 1 covers 16 columns; lane 4 q' + p' of it addresses key row q', columns 4 p' .. 4 p' + 3.
  // The LDS reads are inline asm: the compiler orders a builtin transposed read behind ALL outstanding LDS-DMA
  // (s_waitcnt vmcnt(0)), which would serialise the ring; with asm reads the waits are the counted ones below.
  const unsigned smem_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  int pa_off[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int row = 64 * qh + 32 * a + lq;
#pragma unroll
    for (int st = 0; st < 4; ++st) pa_off[a][st] = row * 128 + (((2 * st + kg) ^ ((row >> 1) & 7)) << 4);
  }
  const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;
  int vbase[4];         // byte offset of this lane's 8 bytes for key-step 0, low half, per 32-column block
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = 128 * ch + 32 * c + 16 * tg + 4 * tp;
    vbase[c] = (8 * kg + tq) * (CW * 2) + ((((col >> 3) ^ (tq << 2)) << 4) | ((col & 7) << 1));
  }

  auto compute = [&](int stage) {
    const unsigned sb = smem_base + stage * SB;
    PvFrags fa, fb;
    pv_load<0>(sb, pa_off, vbase, fa);
    pv_load<1>(sb, pa_off, vbase, fb);
    const bool mm = !(p.debug & 1);
    pv_wait<10>(fa); if (mm) pv_mma(fa, acc);
    pv_load<2>(sb, pa_off, vbase, fa);
    pv_wait<10>(fb); if (mm) pv_mma(fb, acc);
    pv_load<3>(sb, pa_off, vbase, fb);
    pv_wait<10>(fa); if (mm) pv_mma(fa, acc);
    pv_wait<0>(fb); if (mm) pv_mma(fb, acc);
  };
  if constexpr (PC) {
    // both roles pass the same ntl barriers: barrier j = "tile j landed, tile j - 1 is no longer read"
    if (loader) {
      if (ntl > 0) issue(0);
      if (ntl > 1) issue(1);
      int stage = 0;
      for (int j = 0; j < ntl; ++j) {
        if (j + 1 < ntl) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int nxt = stage == 0 ? 2 : stage - 1;
        if (j + 2 < ntl) issue(nxt);
        stage = stage == 2 ? 0 : stage + 1;
      }
      return;
    }
    int stage = 0;
    for (int j = 0; j < ntl; ++j) {
      __builtin_amdgcn_s_barrier();
      compute(stage);
      stage = stage == 2 ? 0 : stage + 1;
    }
  } else {
  if (ntl > 0) issue(0);
  if (ntl > 1) issue(1);
  int stage = 0;
  for (int j = 0; j < ntl; ++j) {
    if (j + 1 < ntl) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int nxt = stage == 0 ? 2 : stage - 1;
    if (j + 2 < ntl && !(p.debug & 2)) issue(nxt);
    compute(stage);
    stage = stage == 2 ? 0 : stage + 1;
  }
  }

  // slab[g][q][c]: accumulator row (r & 3) + 8 (r >> 2) + 4 kg is the query, the lane is the column
  float* slab = p.slabs + (long)g * p.Lqp * p.DV;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = q0 + 64 * qh + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (q < p.Lq) {
#pragma unroll
        for (int c = 0; c < 4; ++c) slab[(long)q * p.DV + c0 + 128 * ch + 32 * c + lq] = acc[a][c][r];
      }
    }
}

struct GpCombine {
  const float* slabs; int groups; const float* lpart; int nrows; int Lq, Lqp, DV;
  const e16* ua; int ldua; const e16* ub; int ldub; int usplit;
  e16* out; int ldo;
  const rmem_attn_chunk* rows; float* mass; int T;
  const float* dw; int H, W;        // optional: depth-wise 5x5 (weights [25][DV]) applied to the gated output in the same launch
  long ua_cs, ub_cs, out_cs, mass_cs, ws_cs; int rows_cs;      // per-clip strides (elements; ws_cs bytes), clip = blockIdx.z
};

__device__ __forceinline__ void gp_select_clip(GpCombine& p, int clip) {
  const long wf = clip * (p.ws_cs >> 2);
  p.slabs += wf; p.lpart += wf;
  p.ua += clip * p.ua_cs;
  if (p.ub) p.ub += clip * p.ub_cs;
  p.out += clip * p.out_cs;
  if (p.rows) p.rows += clip * p.rows_cs;
  if (p.mass) p.mass += clip * p.mass_cs;
}

// The gated value's store rounding, the same function in both combine kernels: the product rounded to fp32, then to e16.  Left to
// the compiler, the half flavour folds the last multiply into v_fma_mixlo/hi_f16 for some of a thread's 8 columns and converts the
// others with v_cvt_pk_f16_f32 -- a different choice in each kernel, and on MI355X the fused depth-wise path then was not
// bit-identical to k_gp_combine + rmem_dwconv5x5 (test_gated_attn_clips_vs_reference[empty-groups-float16]).  The empty asm keeps
// the product out of the conversion's pattern; bfloat16 has no such instruction and compiles as before.
__device__ __forceinline__ e16 gp_store_round(float x) {
#ifdef RMEM_F16
  asm("" : "+v"(x));
#endif
  return (e16)x;
}

// out[q, c] = (sum_g slab[g][q][c]) / l[q] * U[q][c]; thread = 8 columns of one query
__global__ __launch_bounds__(256) void k_gp_combine(GpCombine p) {
  gp_select_clip(p, blockIdx.z);
  const int vpr = p.DV / 8;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)p.Lq * vpr) return;
  const int q = (int)(i / vpr), c = (int)(i - (long)q * vpr) * 8;
  float l = 0.f;
  for (int r = 0; r < p.nrows; ++r) l += p.lpart[(long)r * p.Lqp + q];
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < p.groups; ++g) {
    const float* s = p.slabs + ((long)g * p.Lqp + q) * p.DV + c;
    const f32x4 a = *reinterpret_cast<const f32x4*>(s), b = *reinterpret_cast<const f32x4*>(s + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] += a[j]; v[4 + j] += b[j]; }
  }
  const float inv = 1.f / l;
  e16x8 o;
  if (c < p.usplit) {
    const e16x8 u = *reinterpret_cast<const e16x8*>(p.ua + (long)q * p.ldua + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = gp_store_round(v[j] * inv * (float)u[j]);
  } else if (p.ub) {
    const e16x8 u = *reinterpret_cast<const e16x8*>(p.ub + (long)q * p.ldub + (c - p.usplit));
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = gp_store_round(v[j] * inv * (float)u[j]);
  } else {                                          // torch.ones_like(curr_U) half of layer 0 (transformer.py:1117-1118)
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = gp_store_round(v[j] * inv);
  }
  *reinterpret_cast<e16x8*>(p.out + (long)q * p.ldo + c) = o;
}

// combine + depth-wise 5x5 in one launch (attention.py:208-210: outputs * U -> dw_conv): a tile of 8 x 16 queries x 64 value
// columns with its 2-pixel halo is combined ONCE into LDS (e16, the rounding the two-launch path stores), then the 25 taps
// read LDS.  Saves the [Lq, DV] round trip and a launch per attention call.
constexpr int CT_H = 8, CT_W = 16, CT_C = 64, CT_HW = (CT_H + 4) * (CT_W + 4);
__global__ __launch_bounds__(256) void k_gp_combine_dwconv(GpCombine p) {
  __shared__ __attribute__((aligned(16))) e16 tile[CT_HW * CT_C];
  __shared__ __attribute__((aligned(16))) float wl[25 * CT_C];
  __shared__ float inv_l[CT_HW];
  const int tid = threadIdx.x;
  gp_select_clip(p, blockIdx.z);
  const int tiles_x = (p.W + CT_W - 1) / CT_W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int c0 = blockIdx.y * CT_C;
  for (int i = tid; i < 25 * CT_C; i += 256) wl[i] = p.dw[(i / CT_C) * p.DV + c0 + (i % CT_C)];
  for (int i = tid; i < CT_HW; i += 256) {
    const int hy = i / (CT_W + 4), hx = i - hy * (CT_W + 4);
    const int gy = ty * CT_H + hy - 2, gx = tx * CT_W + hx - 2;
    float v = 0.f;
    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
      const int q = gy * p.W + gx;
      float l = 0.f;
      for (int r = 0; r < p.nrows; ++r) l += p.lpart[(long)r * p.Lqp + q];
      v = 1.f / l;
    }
    inv_l[i] = v;
  }
  __syncthreads();
  const e16* up = c0 < p.usplit ? p.ua + c0 : (p.ub ? p.ub + (c0 - p.usplit) : nullptr);
  const int ldu = c0 < p.usplit ? p.ldua : p.ldub;
  for (int i = tid; i < CT_HW * (CT_C / 8); i += 256) {
    const int pix = i >> 3, ch8 = i & 7;
    const int hy = pix / (CT_W + 4), hx = pix - hy * (CT_W + 4);
    const int gy = ty * CT_H + hy - 2, gx = tx * CT_W + hx - 2;
    e16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
      const int q = gy * p.W + gx;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int g = 0; g < p.groups; ++g) {
        const float* sp = p.slabs + ((long)g * p.Lqp + q) * p.DV + c0 + ch8 * 8;
        const f32x4 a = *reinterpret_cast<const f32x4*>(sp), b = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] += a[j]; v[4 + j] += b[j]; }
      }
      const float inv = inv_l[pix];
      if (up) {
        const e16x8 u = *reinterpret_cast<const e16x8*>(up + (long)q * ldu + ch8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = gp_store_round(v[j] * inv * (float)u[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = gp_store_round(v[j] * inv);
      }
    }
    *reinterpret_cast<e16x8*>(&tile[pix * CT_C + ch8 * 8]) = o;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CT_H * CT_W * (CT_C / 8) / 256; ++k) {
    const int item = tid + 256 * k;
    const int ch8 = item & 7, pp = item >> 3;
    const int oy = pp / CT_W, ox = pp - oy * CT_W;
    const int gy = ty * CT_H + oy, gx = tx * CT_W + ox;
    if (gy >= p.H || gx >= p.W) continue;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx)                   // dx outer, dy inner: the summation order of k_dwconv5 (bit-identical)
#pragma unroll
      for (int dy = 0; dy < 5; ++dy) {
        const e16x8 d = *reinterpret_cast<const e16x8*>(&tile[((oy + dy) * (CT_W + 4) + ox + dx) * CT_C + ch8 * 8]);
        const float* wt = &wl[(dy * 5 + dx) * CT_C + ch8 * 8];
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt), w1 = *reinterpret_cast<const f32x4*>(wt + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j] += (float)d[j] * w0[j]; acc[4 + j] += (float)d[4 + j] * w1[j]; }
      }
    e16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (e16)acc[j];
    *reinterpret_cast<e16x8*>(p.out + ((long)gy * p.W + gx) * p.ldo + c0 + ch8 * 8) = o;
  }
}

// mass[q][t] = sum of the row sums of frame t / total (transformer.py:1185-1192 with one head); grid = (query blocks, T)
__global__ __launch_bounds__(256) void k_gp_mass(GpCombine p) {
  gp_select_clip(p, blockIdx.z);
  const int q = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (q >= p.Lq) return;
  float l = 0.f, lt = 0.f;
  for (int r = 0; r < p.nrows; ++r) {
    const float v = p.lpart[(long)r * p.Lqp + q];
    l += v;
    lt += p.rows[r].t == t ? v : 0.f;
  }
  p.mass[(long)q * p.T + t] = lt / l;
}

struct GpPlan { int Lqp, Lp, ldp, nrows, groups, rpg; size_t off_l, off_p, off_s, total; };

GpPlan plan(int Lq, int DV, int frames, int keys_per_frame, int nrows, int nclips = 1) {
  GpPlan g;
  g.Lqp = (Lq + QT - 1) / QT * QT;
  g.Lp = (keys_per_frame + KT - 1) / KT * KT;
  g.ldp = frames * g.Lp;
  g.nrows = nrows;
  const int tiles = (g.Lqp / QT) * (DV / CW) * (nclips > 0 ? nclips : 1);
  int groups = tiles >= 256 ? 1 : 256 / tiles;      // about one workgroup per CU; the key-tile stream is cut evenly
  const int max_tiles = frames * (g.Lp / KT);
  if (groups > 8) groups = 8;
  if (groups > max_tiles) groups = max_tiles;
  g.rpg = 0;
  g.groups = groups;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  g.off_l = al((size_t)nrows * g.Lqp * 4);
  g.off_p = g.off_l + al((size_t)nrows * g.Lqp * 4);
  g.off_s = g.off_p + al((size_t)g.Lqp * g.ldp * 2);
  g.total = g.off_s + al((size_t)g.groups * g.Lqp * DV * 4) + 256;      // + the launch-wide guard word (clip 0's block carries it)
  return g;
}

int check_common(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int Lq, int DV, const void* ua, int ldua,
                 const void* ub, int ldub, int usplit, const void* out, int ldo, const void* ws, const char* who) {
  RMEM_REQUIRE(q && k && v && ua && out && ws, "rmem_gated_attn: null argument");
  RMEM_REQUIRE(Lq > 0 && DV >= CW && DV % CW == 0 && DV <= 2048, "rmem_gated_attn: DV must be a multiple of 256 (<= 2048)");
  RMEM_REQUIRE(ldq >= DQ && ldk >= DQ && ldv >= DV && ldo >= DV, "rmem_gated_attn: leading dimension too small (d_att is 128)");
  RMEM_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && ldua % 8 == 0 && (!ub || ldub % 8 == 0),
               "rmem_gated_attn: leading dimensions must be multiples of 8 elements");
  RMEM_REQUIRE(usplit > 0 && usplit % 8 == 0 && usplit <= DV && ldua >= usplit && (!ub || ldub >= DV - usplit),
               "rmem_gated_attn: bad gate split");
  RMEM_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)v % 16) == 0 && ((uintptr_t)ua % 16) == 0 &&
               ((uintptr_t)ub % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)ws % 256) == 0,
               "rmem_gated_attn: pointers must be 16-byte aligned (workspace 256)");
  (void)who;
  return 0;
}

template <int MODE>
void launch_all(GpParams& p, const GpPlan& g, GpCombine& c, bool timed, double flops, hipStream_t s) {
  const dim3 sg(p.nq, p.nrows, p.nclips);
  // Softmax reference.  The exact row maximum costs a whole pass over Q K^T (pass 0: 40 % of the score side).  Softmax is invariant
  // under the reference, and bf16 / fp32 keep their relative precision whatever the offset, so pass 0 only SAMPLES the keys (one tile
  // per table row; window mode: the tiles holding the queries' own positions -- always inside their window): P = 2^(S - m_sample) may
  // exceed 1, which is harmless until it leaves the fp32 range.  Pass 1 raises a flag when any score lies more than 2^64 above the
  // reference (or no reference was sampled); the exact pass 0 + pass 1 follow in the same stream and return at once unless it is set
  // (graph-capturable: no host decision).  RMEM_GP_SAMPLE=0: always the exact two passes.
#ifdef RMEM_F16
  // IEEE half holds P only up to 2^16: a sampled reference would need a guard so tight that it fires on ordinary data -- the
  // half flavour keeps the exact two passes (as its memory read always takes the SAFE pass, attention.hip)
  static const bool sample = false;
#else
  static const bool sample = rmem_env_int("RMEM_GP_SAMPLE", 1) != 0;
#endif
  unsigned* flag = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(p.mpart) + g.total - 256);
  if (sample) {
    (void)hipMemsetAsync(flag, 0, 4, s);      // (a failure surfaces in rmem_check_launch after the launches)
    GpParams ps = p;
    ps.sample = 1; ps.flag = flag; ps.gate = nullptr;
    hipLaunchKernelGGL((k_gp_scores<MODE, 0>), sg, dim3(256), 0, s, ps);
    hipLaunchKernelGGL((k_gp_scores<MODE, 1>), sg, dim3(256), 0, s, ps);
    p.gate = flag;
  }
  p.sample = 0; p.flag = nullptr;
  hipLaunchKernelGGL((k_gp_scores<MODE, 0>), sg, dim3(256), 0, s, p);
  hipLaunchKernelGGL((k_gp_scores<MODE, 1>), sg, dim3(256), 0, s, p);
  const dim3 pg(p.nq * p.ncs * p.groups * p.nclips);
  constexpr int PM = MODE == 1 ? 1 : 0;
  const int slot = timed ? rmem_prof_begin(RMEM_PROF_GATED_PV, s, flops) : -1;      // rmem_gated_profile_start: bench.py's DeAOT roofline leg
  // loader waves + MFMA waves (default; RMEM_GP_PC=0: every wave does both).  Measured at cfg 2, T = 9, 8 clips per launch: 610 -> 479 us
  // per launch (671 -> 858 TFLOP/s), the DeAOT workload 1670 -> 1735 frames/s; same MFMA order, so the outputs are bit-identical
  static const bool pc = rmem_env_int("RMEM_GP_PC", 1) != 0;
  if (slot >= 0) {
    if (pc) hipLaunchKernelGGL((k_gp_pv<PM, true, true>), pg, dim3(512), 0, s, p);
    else hipLaunchKernelGGL((k_gp_pv<PM, true>), pg, dim3(256), 0, s, p);
    rmem_prof_end(RMEM_PROF_GATED_PV, slot, s);
  } else {
    if (pc) hipLaunchKernelGGL((k_gp_pv<PM, false, true>), pg, dim3(512), 0, s, p);
    else hipLaunchKernelGGL((k_gp_pv<PM, false>), pg, dim3(256), 0, s, p);
  }
  if (c.dw) hipLaunchKernelGGL(k_gp_combine_dwconv, dim3(((c.W + CT_W - 1) / CT_W) * ((c.H + CT_H - 1) / CT_H), c.DV / CT_C, p.nclips), dim3(256), 0, s, c);
  else hipLaunchKernelGGL(k_gp_combine, dim3((unsigned)(((long)c.Lq * (c.DV / 8) + 255) / 256), 1, p.nclips), dim3(256), 0, s, c);
  if (c.mass) hipLaunchKernelGGL(k_gp_mass, dim3((c.Lq + 255) / 256, c.T, p.nclips), dim3(256), 0, s, c);
  (void)g;
}

}  // namespace

#ifndef RMEM_F16
extern "C" size_t rmem_gated_attn_workspace_bytes(int Lq, int DV, int frames, int keys_per_frame, int nrows) {
  if (Lq <= 0 || DV < CW || DV % CW || frames < 1 || keys_per_frame < 1 || nrows < 1 || nrows > MAX_ROWS) return 0;
  return plan(Lq, DV, frames, keys_per_frame, nrows).total;       // worst case over the clip count (1 clip: most key groups)
}
#endif

extern "C" int RMEM_API(rmem_gated_attn_clips)(const void* q, int ldq, const void* k_bank, long long k_slot_stride, int ldk, const void* v_bank,
                               long long v_slot_stride, int ldv, const rmem_attn_chunk* chunks, int nchunks, int frames,
                               int keys_per_frame, const float* pe_cur, const float* pe_mem, int Lq, int DV, const void* u_a,
                               int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, float* attn_mass,
                               const float* dw_w_t, int H, int W, int nclips, void* workspace, void* stream);
extern "C" int RMEM_API(rmem_gated_attn)(const void* q, int ldq, const void* k_bank, long long k_slot_stride, int ldk, const void* v_bank,
                               long long v_slot_stride, int ldv, const rmem_attn_chunk* chunks, int nchunks, int frames,
                               int keys_per_frame, const float* pe_cur, const float* pe_mem, int Lq, int DV, const void* u_a,
                               int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, float* attn_mass,
                               const float* dw_w_t, int H, int W, void* workspace, void* stream) {
  return RMEM_API(rmem_gated_attn_clips)(q, ldq, k_bank, k_slot_stride, ldk, v_bank, v_slot_stride, ldv, chunks, nchunks, frames, keys_per_frame,
                                         pe_cur, pe_mem, Lq, DV, u_a, ldua, u_b, ldub, usplit, out, ldo, attn_mass, dw_w_t, H, W, 1, workspace, stream);
}

extern "C" int RMEM_API(rmem_gated_attn_clips)(const void* q, int ldq, const void* k_bank, long long k_slot_stride, int ldk, const void* v_bank,
                               long long v_slot_stride, int ldv, const rmem_attn_chunk* chunks, int nchunks, int frames,
                               int keys_per_frame, const float* pe_cur, const float* pe_mem, int Lq, int DV, const void* u_a,
                               int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, float* attn_mass,
                               const float* dw_w_t, int H, int W, int nclips, void* workspace, void* stream) {
  RMEM_REQUIRE(nclips >= 1 && nclips <= 64, "rmem_gated_attn: 1..64 clips");
  if (check_common(q, ldq, k_bank, ldk, v_bank, ldv, Lq, DV, u_a, ldua, u_b, ldub, usplit, out, ldo, workspace, "rmem_gated_attn")) return -1;
  RMEM_REQUIRE(frames >= 1 && keys_per_frame >= 1, "rmem_gated_attn: frames and keys_per_frame must be >= 1");
  RMEM_REQUIRE(nchunks >= 1 && nchunks <= MAX_ROWS, "rmem_gated_attn: 1 <= nchunks <= 64");
  RMEM_REQUIRE(chunks || frames == 1, "rmem_gated_attn: more than one key frame needs a chunk table");
  RMEM_REQUIRE(!attn_mass || (chunks && frames <= 32), "rmem_gated_attn: the mass output needs a chunk table and <= 32 frames");
  RMEM_REQUIRE(!pe_mem || chunks, "rmem_gated_attn: pe_mem needs a chunk table");
  RMEM_REQUIRE(k_slot_stride % 8 == 0 && v_slot_stride % 8 == 0, "rmem_gated_attn: slot strides must be multiples of 8 elements");
  RMEM_REQUIRE(!dw_w_t || (H > 0 && W > 0 && H * W == Lq && usplit % 64 == 0), "rmem_gated_attn: the fused depth-wise conv needs H * W == Lq and usplit % 64 == 0");
  GpParams p = {};
  p.q = (const e16*)q; p.ldq = ldq; p.k = (const e16*)k_bank; p.k_slot_stride = k_slot_stride; p.ldk = ldk;
  p.v = (const e16*)v_bank; p.v_slot_stride = v_slot_stride; p.ldv = ldv;
  p.rows = chunks; p.lk = keys_per_frame;
  int nrows = nchunks;
  if (!chunks) {                 // one key frame cut into ranges that start on tile boundaries
    p.per = ((keys_per_frame + nchunks - 1) / nchunks + KT - 1) / KT * KT;
    nrows = (keys_per_frame + p.per - 1) / p.per;
  }
  p.nrows = nrows;
  const GpPlan g = plan(Lq, DV, frames, keys_per_frame, nrows, nclips);
  // clips: [clip][Lq rows] layouts of q / gates / out; one-frame keys and values [clip][keys]; the bank through global slots
  p.nclips = nclips; p.q_cs = (long)Lq * ldq; p.k_cs = chunks ? 0 : (long)keys_per_frame * ldk; p.v_cs = chunks ? 0 : (long)keys_per_frame * ldv;
  p.rel_cs = 0; p.ws_cs = (long)g.total; p.rows_cs = nchunks;
  p.pe_cur = pe_cur; p.pe_mem = pe_mem; p.Lq = Lq; p.Lqp = g.Lqp; p.Lp = g.Lp; p.ldp = g.ldp;
  RMEM_REQUIRE((long)g.Lqp * g.ldp < (1L << 31), "rmem_gated_attn: probability matrix exceeds 2^31 elements");
  char* ws = (char*)workspace;
  p.mpart = (float*)ws; p.lpart = (float*)(ws + g.off_l); p.P = (e16*)(ws + g.off_p); p.slabs = (float*)(ws + g.off_s);
  p.qscale = LOG2E / sqrtf((float)DQ);
  p.DV = DV; p.nq = g.Lqp / QT; p.ncs = DV / CW; p.groups = g.groups; p.rows_per_group = g.rpg;
  { static const int dbg = rmem_env_int("RMEM_GP_DEBUG", 0); p.debug = dbg; }
  GpCombine c = {};
  c.slabs = p.slabs; c.groups = g.groups; c.lpart = p.lpart; c.nrows = nrows; c.Lq = Lq; c.Lqp = g.Lqp; c.DV = DV;
  c.ua = (const e16*)u_a; c.ldua = ldua; c.ub = (const e16*)u_b; c.ldub = ldub; c.usplit = usplit;
  c.out = (e16*)out; c.ldo = ldo; c.rows = chunks; c.mass = attn_mass; c.T = frames;
  c.dw = dw_w_t; c.H = H; c.W = W;
  c.ua_cs = (long)Lq * ldua; c.ub_cs = (long)Lq * ldub; c.out_cs = (long)Lq * ldo; c.mass_cs = (long)Lq * frames; c.ws_cs = (long)g.total;
  c.rows_cs = nchunks;
  hipStream_t s = (hipStream_t)stream;
  const double flops = 2.0 * (double)Lq * (double)frames * (double)keys_per_frame * (double)DV * nclips;
  if (chunks) launch_all<1>(p, g, c, true, flops, s);
  else launch_all<0>(p, g, c, false, flops, s);
  return rmem_check_launch("rmem_gated_attn");
}

extern "C" int RMEM_API(rmem_local_gated_attn_clips)(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel,
                                     int ldrel, int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub,
                                     int usplit, void* out, int ldo, const float* dw_w_t, int nclips, void* workspace, void* stream);
extern "C" int RMEM_API(rmem_local_gated_attn)(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel,
                                     int ldrel, int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub,
                                     int usplit, void* out, int ldo, const float* dw_w_t, void* workspace, void* stream) {
  return RMEM_API(rmem_local_gated_attn_clips)(q, ldq, k, ldk, v, ldv, rel, ldrel, H, W, DV, u_a, ldua, u_b, ldub, usplit, out, ldo, dw_w_t, 1,
                                               workspace, stream);
}

extern "C" int RMEM_API(rmem_local_gated_attn_clips)(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel,
                                     int ldrel, int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub,
                                     int usplit, void* out, int ldo, const float* dw_w_t, int nclips, void* workspace, void* stream) {
  RMEM_REQUIRE(nclips >= 1 && nclips <= 64, "rmem_local_gated_attn: 1..64 clips");
  const int L = H * W;
  if (check_common(q, ldq, k, ldk, v, ldv, L, DV, u_a, ldua, u_b, ldub, usplit, out, ldo, workspace, "rmem_local_gated_attn")) return -1;
  RMEM_REQUIRE(rel && H > 0 && W > 0 && W < 32768 && ldrel >= WIN * WIN, "rmem_local_gated_attn: bad rel / H / W");
  GpParams p = {};
  p.q = (const e16*)q; p.ldq = ldq; p.k = (const e16*)k; p.ldk = ldk; p.v = (const e16*)v; p.ldv = ldv;
  p.lk = L;
  // key ranges (= score workgroups per query tile and clip): 8 for a single clip; with several clips per launch the grid is full
  // anyway and a workgroup's fixed prologue (Q fragments, window coordinates) is spread over more key tiles
  // (8 clips, cfg 2: 8 -> 4 ranges, DeAOT workload 1757 -> 1782 frames/s)
  static const int rows_env = rmem_env_int("RMEM_GP_LOCAL_ROWS", 0);      // kernel experiments only
  const int tiles_q = ((L + QT - 1) / QT) * nclips;
  const int want = rows_env > 0 ? rows_env : max(2, min(8, (448 + tiles_q - 1) / tiles_q));
  p.per = ((L + want - 1) / want + KT - 1) / KT * KT;
  p.nrows = (L + p.per - 1) / p.per;
  const GpPlan g = plan(L, DV, 1, L, p.nrows, nclips);
  p.nclips = nclips; p.q_cs = (long)L * ldq; p.k_cs = (long)L * ldk; p.v_cs = (long)L * ldv; p.rel_cs = (long)L * ldrel; p.ws_cs = (long)g.total;
  p.rows_cs = 0;
  p.Lq = L; p.Lqp = g.Lqp; p.Lp = g.Lp; p.ldp = g.ldp;
  char* ws = (char*)workspace;
  p.mpart = (float*)ws; p.lpart = (float*)(ws + g.off_l); p.P = (e16*)(ws + g.off_p); p.slabs = (float*)(ws + g.off_s);
  p.qscale = LOG2E / sqrtf((float)DQ);
  p.H = H; p.W = W; p.rel = rel; p.ldrel = ldrel;
  p.DV = DV; p.nq = g.Lqp / QT; p.ncs = DV / CW; p.groups = g.groups; p.rows_per_group = g.rpg;
  { static const int dbg = rmem_env_int("RMEM_GP_DEBUG", 0); p.debug = dbg; }
  GpCombine c = {};
  c.slabs = p.slabs; c.groups = g.groups; c.lpart = p.lpart; c.nrows = p.nrows; c.Lq = L; c.Lqp = g.Lqp; c.DV = DV;
  c.ua = (const e16*)u_a; c.ldua = ldua; c.ub = (const e16*)u_b; c.ldub = ldub; c.usplit = usplit;
  c.out = (e16*)out; c.ldo = ldo;
  RMEM_REQUIRE(!dw_w_t || usplit % 64 == 0, "rmem_local_gated_attn: the fused depth-wise conv needs usplit % 64 == 0");
  c.dw = dw_w_t; c.H = H; c.W = W;
  c.ua_cs = (long)L * ldua; c.ub_cs = (long)L * ldub; c.out_cs = (long)L * ldo; c.mass_cs = 0; c.ws_cs = (long)g.total; c.rows_cs = 0;
  launch_all<2>(p, g, c, false, 0.0, (hipStream_t)stream);
  return rmem_check_launch("rmem_local_gated_attn");
}
