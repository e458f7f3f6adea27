// Traced polygon rings simplified on the device (include/rmem.h, rmem_polygon_simplify): Douglas-Peucker in exact 64-bit integer
// arithmetic on the ring table of rmem_label_polygons, so that tens of vertices per object leave the device, not every corner of
// a pixel staircase (polygons.py: simplify, trace_label_stack(tolerance=...)).  int32 tables in, int32 tables out: built once.
//
// The recursion of the contract is run breadth first.  Every vertex that is neither kept nor dropped knows its segment (lo, hi),
// the kept vertices on either side.  One round: every such vertex computes its key against its segment, the segment's arg-max
// (largest key, then smallest index) is found, and either the winner is kept and the others move into (lo, winner) or
// (winner, hi), or the whole segment is dropped.  Segments are independent, so the rounds reach exactly the set the recursion
// keeps; a ring needs as many rounds as its recursion is deep, at most its vertex count.  No workgroup waits for another: a ring
// lives in one wave (at most kShortMax vertices: a vertex per lane, the state in registers, the arg-max a segmented scan by
// shuffles, a fixed tree) or in one workgroup (longer: the state in the workspace, the arg-max a segmented scan inside every
// wave and then integer atomicMax of the key and atomicMin of the index among the maxima, which commute).  Both give the same
// bytes.  Integer arithmetic only, every loop bounded, every index from device memory checked, no host sync.
//
//   k_simp_count       per tile of 2048 rings: every ring's checked vertex count (0: a bad row) and the tile's sum.
//   k_simp_head        one workgroup: R, V and the status of the input, the scan of the tiles' sums; the header (R in effect, V,
//                      status) to the workspace.
//   k_simp_apply       per tile: the base of every ring's state in the workspace (the scan of the counts).
//   k_simp_short       one wave per ring of at most kShortMax vertices (grid-stride over r < R): coordinates checked, anchors,
//                      rounds; the kept set as a 64-bit mask and its count.
//   k_simp_long        one workgroup per longer ring (grid-stride over chunks of 256 rings; a thread per ring finds the chunk's
//                      long ones): the same, the kept vertices' ranks by a workgroup scan.
//   k_simp_partial, k_simp_bases, k_simp_apply   the same three steps over the kept counts: every ring's first output vertex;
//                      counts_out.
//   k_simp_emit_short  one wave per ring: the ring's row and its kept vertices.
//   k_simp_emit_long   one workgroup per ring: the same from the ranks.
#include <limits.h>
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
typedef unsigned long long u64;
constexpr int kShortMax = 64;                     // vertices of a ring that one wave holds, a vertex per lane
constexpr int kMaxCoord = 32767;
constexpr int kScanItems = 8;                     // rings per thread of the scans over the rings
constexpr int kScanTile = kThreads * kScanItems;
constexpr int kLongBlocks = 1024;                 // workgroups of the kernels that take a ring each
constexpr int kKept = -2, kDropped = -1;          // state.x of a vertex that left the rounds

struct Layout {
  size_t hdr, cnt, ibase, kc, obase, mask, state, key, idx, bsum, bbad, bytes;      // byte offsets into the workspace
  long long tiles;                                                                  // tiles of one scan over the rings
};
Layout layout(long long MR, long long MV) {
  Layout l;
  l.hdr = 0;
  l.cnt = 16;
  l.ibase = align16(l.cnt + (size_t)MR * 4);
  l.kc = align16(l.ibase + (size_t)MR * 4);
  l.obase = align16(l.kc + (size_t)MR * 4);
  l.mask = align16(l.obase + (size_t)MR * 4);
  l.state = align16(l.mask + (size_t)MR * 8);
  l.key = align16(l.state + (size_t)MV * 8);
  l.idx = align16(l.key + (size_t)MV * 16);
  l.tiles = (MR + kScanTile - 1) / kScanTile;
  l.bsum = align16(l.idx + (size_t)MV * 8);
  l.bbad = align16(l.bsum + (size_t)l.tiles * 8);
  l.bytes = align16(l.bbad + (size_t)l.tiles * 4);
  return l;
}

// key of vertex m against the segment p_i p_j and the segment's threshold: the contract's four cases, every product below 2^62
__device__ __forceinline__ void seg_key(int xi, int yi, int xj, int yj, int xm, int ym, long long T2, u64& key, u64& thr) {
  const long long ax = xj - xi, ay = yj - yi, bx = xm - xi, by = ym - yi;
  const long long L = ax * ax + ay * ay, bb = bx * bx + by * by, t = ax * bx + ay * by;
  const long long cx = xm - xj, cy = ym - yj, cr = ax * by - ay * bx;
  long long k = cr * cr;
  if (t >= L) k = (cx * cx + cy * cy) * L;
  if (t <= 0) k = bb * L;
  if (L == 0) k = bb;
  key = (u64)k;
  thr = (u64)((L == 0 ? T2 : T2 * L) >> 8);
}

// Inclusive scan of (key, idx) over the lanes before this one that share its segment id: the largest key, the smallest index
// among equals.  Segments are runs of consecutive lanes; a lane that takes no part has an id of its own.
__device__ __forceinline__ void seg_scan(int lane, int seg, u64& key, int& idx) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 k2 = __shfl_up(key, o, 64);
    const int i2 = __shfl_up(idx, o, 64), s2 = __shfl_up(seg, o, 64);
    if (lane >= o && s2 == seg) {
      if (k2 > key) {
        key = k2;
        idx = i2;
      } else if (k2 == key) {
        idx = min(idx, i2);
      }
    }
  }
}

__device__ __forceinline__ u64 wave_umax(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

__device__ __forceinline__ bool coord_ok(int x, int y) { return (unsigned)x <= (unsigned)kMaxCoord && (unsigned)y <= (unsigned)kMaxCoord; }
// squared distance to p_0 above, the complement of the index below: the maximum is the farthest vertex, the first of equals
__device__ __forceinline__ u64 anchor_word(int x, int y, int x0, int y0, int m) {
  const long long dx = x - x0, dy = y - y0;
  return ((u64)(dx * dx + dy * dy) << 32) | (u64)(0xffffffffu - (unsigned)m);
}

// a ring row's vertex range, checked against V: the count, or 0
__device__ __forceinline__ int ring_count(const int* __restrict__ rings, int r, int V, int& first) {
  first = rings[8 * (size_t)r + 2];
  const int c = rings[8 * (size_t)r + 3];
  return (first >= 0 && c >= 1 && (long long)first + c <= V) ? c : 0;
}

// ------------------------------------------------------------------------------------------------------------------- header
// the rings the call works on and the status it starts from: the same words in every workgroup of k_simp_count and in k_simp_head
__device__ __forceinline__ int rings_in_effect(const int* __restrict__ counts, long long MR, long long MV, int& V, int& status) {
  const int R = counts[1], st_in = counts[3];
  V = counts[2];
  status = st_in;
  if (st_in != 0) return 0;
  if (R < 0 || R > MR || V < 0 || V > MV) {
    status = RMEM_SIMPLIFY_ST_TABLE;
    return 0;
  }
  return R;
}

// Device-wide exclusive scan over the rings in three steps, as label_polygons.hip scans its edges: every tile of kScanTile rings is
// summed, one workgroup scans the tiles' sums, every tile is scanned again from its base.  Sums in 64 bits.
__global__ __launch_bounds__(kThreads) void k_simp_count(const int* __restrict__ rings, const int* __restrict__ counts, long long MR, long long MV,
                                                         int* __restrict__ cnt, long long* __restrict__ bsum, int* __restrict__ bbad) {
  __shared__ long long sh[kWaves];
  int V, status;
  const int Re = rings_in_effect(counts, MR, MV, V, status);
  const long long tiles = ((long long)Re + kScanTile - 1) / kScanTile;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long i0 = t * kScanTile + (long long)threadIdx.x * kScanItems;
    long long sum = 0;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      if (i0 + k < Re) {
        int first;
        const int c = ring_count(rings, (int)(i0 + k), V, first);
        cnt[i0 + k] = c;
        bad |= c == 0;
        sum += c;
      }
    }
    long long tot;
    block_incl_scan(sum, sh, tot);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
      bsum[t] = tot;
      bbad[t] = bad;
    }
  }
}

// one workgroup: the tiles' sums scanned in place; what `total` says goes to the caller
__device__ __forceinline__ long long scan_tiles(long long* __restrict__ bsum, long long tiles, long long* sh) {
  long long carry = 0;
  for (long long b = 0; b < tiles; b += kThreads) {
    const long long i = b + threadIdx.x;
    const long long v = i < tiles ? bsum[i] : 0;
    long long tot;
    const long long inc = block_incl_scan(v, sh, tot);
    if (i < tiles) bsum[i] = carry + inc - v;
    carry += tot;
  }
  return carry;
}

__global__ __launch_bounds__(kThreads) void k_simp_head(const int* __restrict__ counts, long long MR, long long MV, long long* __restrict__ bsum,
                                                        const int* __restrict__ bbad, int* __restrict__ hdr) {
  __shared__ long long sh[kWaves];
  int V, status;
  int Re = rings_in_effect(counts, MR, MV, V, status);
  const long long tiles = ((long long)Re + kScanTile - 1) / kScanTile;
  int bad = 0;
  for (long long i = threadIdx.x; i < tiles; i += kThreads) bad |= bbad[i];
  const long long total = scan_tiles(bsum, tiles, sh);
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    if (total > MV) {                                               // rings that share vertices: the state and the output would not fit
      status = RMEM_SIMPLIFY_ST_TABLE;
      Re = 0;
    } else if (bad) {
      status |= RMEM_SIMPLIFY_ST_RING;
    }
    hdr[0] = Re;
    hdr[1] = V;
    hdr[2] = status;
    hdr[3] = 0;
  }
}

// per tile: the sum of in[] (negative entries count as 0), for the second scan
__global__ __launch_bounds__(kThreads) void k_simp_partial(const int* __restrict__ hdr, const int* __restrict__ in, long long* __restrict__ bsum) {
  __shared__ long long sh[kWaves];
  const int R = hdr[0];
  const long long tiles = ((long long)R + kScanTile - 1) / kScanTile;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long i0 = t * kScanTile + (long long)threadIdx.x * kScanItems;
    long long sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
      if (i0 + k < R) sum += max(in[i0 + k], 0);
    long long tot;
    block_incl_scan(sum, sh, tot);
    if (threadIdx.x == 0) bsum[t] = tot;
  }
}

// per tile: out[] = the tile's base + the exclusive scan of in[] inside the tile
__global__ __launch_bounds__(kThreads) void k_simp_apply(const int* __restrict__ hdr, const int* __restrict__ in, const long long* __restrict__ bsum,
                                                         int* __restrict__ out) {
  __shared__ long long sh[kWaves];
  const int R = hdr[0];
  const long long tiles = ((long long)R + kScanTile - 1) / kScanTile;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long i0 = t * kScanTile + (long long)threadIdx.x * kScanItems;
    int c[kScanItems];
    long long sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      c[k] = i0 + k < R ? max(in[i0 + k], 0) : 0;
      sum += c[k];
    }
    long long tot;
    long long at = bsum[t] + block_incl_scan(sum, sh, tot) - sum;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      if (i0 + k < R) out[i0 + k] = (int)min(at, (long long)INT_MAX);
      at += c[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------- rings that one wave holds
__global__ __launch_bounds__(kThreads) void k_simp_short(const int* __restrict__ rings, const int* __restrict__ verts, int* hdr,
                                                         const int* __restrict__ cnt, int T, int* __restrict__ kc, u64* __restrict__ mask) {
  const int R = hdr[0], V = hdr[1];
  const int lane = threadIdx.x & 63;
  const long long T2 = (long long)T * T;
  const long long nw = (long long)gridDim.x * kWaves;
  for (long long rr = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); rr < R; rr += nw) {
    const int r = (int)rr;
    int first;
    const int c = min(cnt[r], ring_count(rings, r, V, first));      // both 0 for a bad row
    if (c > kShortMax) continue;
    const bool in = lane < c;
    int x = 0, y = 0;
    if (in) {
      x = verts[2 * ((size_t)first + lane)];
      y = verts[2 * ((size_t)first + lane) + 1];
    }
    if (c < 1 || __any(in && !coord_ok(x, y))) {
      if (lane == 0) {
        kc[r] = 0;
        mask[r] = 0;
        if (c >= 1) atomicOr(hdr + 2, RMEM_SIMPLIFY_ST_RING);       // the head flagged the bad rows
      }
      continue;
    }
    const int x0 = __shfl(x, 0, 64), y0 = __shfl(y, 0, 64);
    const u64 far = wave_umax(in && lane >= 1 ? anchor_word(x, y, x0, y0, lane) : 0);
    const int B = c > 1 ? (int)(0xffffffffu - (unsigned)far) : 0;   // 1..c-1
    bool kept = in && (lane == 0 || lane == B);
    int lo = -1, hi = -1;                                           // hi >= 0: still in the rounds
    if (in && !kept) {
      lo = lane < B ? 0 : B;
      hi = lane < B ? B : c;
    }
    for (int it = 0; it < c; ++it) {                                // a ring's refinement runs at most its vertex count of rounds
      const bool active = hi >= 0;
      if (!__any(active)) break;
      const int li = active ? lo : 0, lj = active && hi < c ? hi : 0;          // hi = c closes the ring: p_c = p_0
      const int xi = __shfl(x, li, 64), yi = __shfl(y, li, 64), xj = __shfl(x, lj, 64), yj = __shfl(y, lj, 64);
      u64 key, thr;
      seg_key(xi, yi, xj, yj, x, y, T2, key, thr);
      int idx = lane;
      if (!active) key = 0;
      seg_scan(lane, active ? lo : -1 - lane, key, idx);
      const int last = active ? hi - 1 : lane;                      // the segment's last vertex holds the scan of all of it
      const u64 best = __shfl(key, last, 64);
      const int w = __shfl(idx, last, 64);
      if (active) {
        if (best > thr) {
          if (lane == w) {
            kept = true;
            lo = hi = -1;
          } else if (lane < w) {
            hi = w;
          } else {
            lo = w;
          }
        } else {
          lo = hi = -1;
        }
      }
    }
    const u64 m = __ballot(kept);
    if (lane == 0) {
      kc[r] = __popcll(m);
      mask[r] = m;
    }
  }
}

// ------------------------------------------------------------------------------------------- rings that one workgroup holds
// what a vertex of a long ring does in every phase of a round: its state, its key against its segment, the scan inside its wave
struct Probe {
  int lo, hi;
  bool active, last;        // last: the last lane of its segment's run in this wave, which speaks for the run
  u64 key, thr;
  int idx;
};
__device__ __forceinline__ Probe probe(const int* __restrict__ verts, size_t first, const int2* st, int c, int m, int lane, long long T2) {
  Probe p;
  p.lo = p.hi = -1;
  if (m < c) {
    const int2 s = st[m];
    if (s.x >= 0 && s.x < m && s.y > m && s.y <= c) {               // anything else has left the rounds
      p.lo = s.x;
      p.hi = s.y;
    }
  }
  p.active = p.hi >= 0;
  p.key = p.thr = 0;
  p.idx = m;
  if (p.active) {
    const size_t i = first + p.lo, j = first + (p.hi < c ? p.hi : 0), k = first + m;
    seg_key(verts[2 * i], verts[2 * i + 1], verts[2 * j], verts[2 * j + 1], verts[2 * k], verts[2 * k + 1], T2, p.key, p.thr);
  }
  const int seg = p.active ? p.lo : -1 - lane;
  seg_scan(lane, seg, p.key, p.idx);
  const int next = __shfl_down(seg, 1, 64);
  p.last = p.active && (lane == 63 || next != seg);
  return p;
}

__device__ __forceinline__ u64 load_u64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int load_int(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void clear_slot(u64* key, int* idx, size_t at) {
  __hip_atomic_store(key + at, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(idx + at, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The rings of chunk .. chunk + kThreads - 1 with more than kShortMax vertices, in ring order, to list; their number.  A thread
// per ring: a workgroup does not walk the table a ring at a time to find the few it works on.
__device__ __forceinline__ int long_rings(const int* __restrict__ cnt, int R, long long chunk, int* list, int* sh) {
  const long long r = chunk + threadIdx.x;
  const int flag = r < R && cnt[r] > kShortMax;
  int tot;
  const int at = block_incl_scan(flag, sh, tot) - flag;
  if (flag) list[at] = (int)r;
  __syncthreads();
  return tot;
}

__global__ __launch_bounds__(kThreads) void k_simp_long(const int* __restrict__ rings, const int* __restrict__ verts, int* hdr,
                                                        const int* __restrict__ cnt, const int* __restrict__ ibase, int T, long long MV,
                                                        int* __restrict__ kc, int2* state, u64* key, int* idx) {
  __shared__ u64 shf[kWaves];
  __shared__ int shs[kWaves];
  __shared__ int list[kThreads];
  const int R = hdr[0], V = hdr[1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long T2 = (long long)T * T;
  for (long long chunk = (long long)blockIdx.x * kThreads; chunk < R; chunk += (long long)gridDim.x * kThreads) {
   const int found = long_rings(cnt, R, chunk, list, shs);          // a thread per ring looks for the chunk's long rings
   for (int j = 0; j < found; ++j) {
    const int r = list[j];
    int first0;
    const int c = min(cnt[r], ring_count(rings, r, V, first0));
    const long long base = ibase[r];
    if (c <= kShortMax || base < 0 || base + c > MV) continue;      // never: the list holds long rings, the head's scan stays within max_verts
    const size_t first = (size_t)first0;
    int2* st = state + base;
    u64* key0 = key + base;                                         // slot of a segment: its lo, in the round's parity
    int* idx0 = idx + base;
    // coordinates and the far anchor
    const int x0 = verts[2 * first], y0 = verts[2 * first + 1];
    int bad = 0;
    u64 far = 0;
    for (int m = threadIdx.x; m < c; m += kThreads) {
      const int x = verts[2 * (first + m)], y = verts[2 * (first + m) + 1];
      bad |= !coord_ok(x, y);
      if (m >= 1) {
        const u64 a = anchor_word(x, y, x0, y0, m);
        far = a > far ? a : far;
      }
    }
    far = wave_umax(far);
    __syncthreads();                                                // the previous ring's readers are done with shf
    if (lane == 0) shf[wave] = far;
    bad = __syncthreads_or(bad);
    if (bad) {
      if (threadIdx.x == 0) {
        kc[r] = 0;
        atomicOr(hdr + 2, RMEM_SIMPLIFY_ST_RING);
      }
      continue;
    }
    far = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) far = shf[k] > far ? shf[k] : far;
    const int B = (int)(0xffffffffu - (unsigned)far);               // 1..c-1, c > kShortMax
    if (B < 1 || B >= c) {                                          // never
      if (threadIdx.x == 0) kc[r] = 0;
      continue;
    }
    for (int m = threadIdx.x; m < c; m += kThreads)
      st[m] = (m == 0 || m == B) ? make_int2(kKept, 0) : m < B ? make_int2(0, B) : make_int2(B, c);
    if (threadIdx.x == 0) {
      clear_slot(key0, idx0, 0);
      clear_slot(key0, idx0, B);
    }
    __syncthreads();
    for (int it = 0; it < c; ++it) {                                // at most the ring's vertex count of rounds
      const size_t par = (it & 1) ? (size_t)MV : 0, other = (it & 1) ? 0 : (size_t)MV;
      for (int mb = 0; mb < c; mb += kThreads) {                    // whole waves: the scan shuffles
        const Probe p = probe(verts, first, st, c, mb + threadIdx.x, lane, T2);
        if (p.last) atomicMax(key0 + par + p.lo, p.key);
      }
      __syncthreads();
      for (int mb = 0; mb < c; mb += kThreads) {
        const Probe p = probe(verts, first, st, c, mb + threadIdx.x, lane, T2);
        if (p.last && p.key == load_u64(key0 + par + p.lo)) atomicMin(idx0 + par + p.lo, p.idx);
      }
      __syncthreads();
      int changed = 0;
      for (int mb = 0; mb < c; mb += kThreads) {
        const int m = mb + threadIdx.x;
        const Probe p = probe(verts, first, st, c, m, lane, T2);
        if (!p.active) continue;
        const u64 best = load_u64(key0 + par + p.lo);
        const int w = load_int(idx0 + par + p.lo);
        if (best > p.thr && w > p.lo && w < p.hi) {                 // w in the segment: always, when best > 0
          if (m == w) {
            st[m] = make_int2(kKept, 0);
            clear_slot(key0 + other, idx0 + other, p.lo);           // the two halves' slots of the next round
            clear_slot(key0 + other, idx0 + other, m);
            changed = 1;
          } else {
            st[m] = m < w ? make_int2(p.lo, w) : make_int2(w, p.hi);
          }
        } else {
          st[m] = make_int2(kDropped, 0);
        }
      }
      if (!__syncthreads_or(changed)) break;                        // no segment split: every one was dropped
    }
    // the kept vertices' ranks, next to their flags
    int carry = 0;
    for (int mb = 0; mb < c; mb += kThreads) {
      const int m = mb + threadIdx.x;
      const int flag = m < c && st[m].x == kKept;
      int tot;
      const int inc = block_incl_scan(flag, shs, tot);
      if (m < c) st[m] = make_int2(flag ? kKept : kDropped, carry + inc - flag);
      carry += tot;
    }
    if (threadIdx.x == 0) kc[r] = carry;
   }
  }
}

// --------------------------------------------------------------------------------------------------------------- output bases
__global__ __launch_bounds__(kThreads) void k_simp_bases(const int* __restrict__ hdr, long long MV, long long* __restrict__ bsum,
                                                         int* __restrict__ counts_out) {
  __shared__ long long sh[kWaves];
  const int R = hdr[0];
  const long long total = scan_tiles(bsum, ((long long)R + kScanTile - 1) / kScanTile, sh);
  if (threadIdx.x == 0) {
    counts_out[0] = hdr[1];
    counts_out[1] = R;
    counts_out[2] = (int)min(total, MV);                            // at most the input's vertices, which fit
    counts_out[3] = hdr[2];
  }
}

// ------------------------------------------------------------------------------------------------------------------- output
__device__ __forceinline__ void emit_row(const int* __restrict__ rings, int r, int t, int base, int kept, int* __restrict__ rings_out) {
  if (t >= 8) return;
  const int* in = rings + 8 * (size_t)r;
  rings_out[8 * (size_t)r + t] = t == 2 ? base : t == 3 ? kept : t == 7 ? in[3] : in[t];
}

__global__ __launch_bounds__(kThreads) void k_simp_emit_short(const int* __restrict__ rings, const int* __restrict__ verts, const int* __restrict__ hdr,
                                                              const int* __restrict__ cnt, const int* __restrict__ kc, const int* __restrict__ obase,
                                                              const u64* __restrict__ mask, long long MV, int* __restrict__ rings_out,
                                                              int* __restrict__ verts_out) {
  const int R = hdr[0], V = hdr[1];
  const int lane = threadIdx.x & 63;
  const long long nw = (long long)gridDim.x * kWaves;
  for (long long rr = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); rr < R; rr += nw) {
    const int r = (int)rr;
    int first;
    const int c = min(cnt[r], ring_count(rings, r, V, first));
    if (c > kShortMax) continue;
    const u64 m = c >= 1 ? mask[r] : 0;
    const int base = obase[r];
    emit_row(rings, r, lane, base, __popcll(m), rings_out);
    if (lane < c && ((m >> lane) & 1)) {
      const long long at = (long long)base + __popcll(m & (((u64)1 << lane) - 1));
      if (at >= 0 && at < MV) {
        verts_out[2 * at] = verts[2 * ((size_t)first + lane)];
        verts_out[2 * at + 1] = verts[2 * ((size_t)first + lane) + 1];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_simp_emit_long(const int* __restrict__ rings, const int* __restrict__ verts, const int* __restrict__ hdr,
                                                             const int* __restrict__ cnt, const int* __restrict__ ibase, const int* __restrict__ kc,
                                                             const int* __restrict__ obase, const int2* __restrict__ state, long long MV,
                                                             int* __restrict__ rings_out, int* __restrict__ verts_out) {
  __shared__ int shs[kWaves];
  __shared__ int list[kThreads];
  const int R = hdr[0], V = hdr[1];
  for (long long chunk = (long long)blockIdx.x * kThreads; chunk < R; chunk += (long long)gridDim.x * kThreads) {
   const int found = long_rings(cnt, R, chunk, list, shs);
   for (int j = 0; j < found; ++j) {
    const int r = list[j];
    int first;
    const int c = min(cnt[r], ring_count(rings, r, V, first));
    const long long sb = ibase[r];
    if (c <= kShortMax || sb < 0 || sb + c > MV) continue;
    const int kept = max(kc[r], 0), base = obase[r];
    emit_row(rings, r, threadIdx.x, base, kept, rings_out);
    if (kept == 0) continue;                                        // a ring with a bad vertex: its state was never written
    const int2* st = state + sb;
    for (int m = threadIdx.x; m < c; m += kThreads) {
      const int2 s = st[m];
      const long long at = (long long)base + s.y;
      if (s.x == kKept && s.y >= 0 && s.y < kept && at < MV) {
        verts_out[2 * at] = verts[2 * ((size_t)first + m)];
        verts_out[2 * at + 1] = verts[2 * ((size_t)first + m) + 1];
      }
    }
   }
  }
}

bool capacities_ok(long long MR, long long MV) { return MR >= 1 && MR <= INT_MAX && MV >= 1 && MV <= INT_MAX; }
}  // namespace

extern "C" int rmem_polygon_simplify_short_max(void) { return kShortMax; }

extern "C" size_t rmem_polygon_simplify_workspace_bytes(long long max_rings, long long max_verts) {
  if (!capacities_ok(max_rings, max_verts)) return 0;
  return layout(max_rings, max_verts).bytes;
}

extern "C" int rmem_polygon_simplify(const int* rings, const int* verts, const int* counts, long long max_rings, long long max_verts,
                                     int tolerance_16ths, void* workspace, size_t workspace_bytes, int* rings_out, int* verts_out,
                                     int* counts_out, void* stream) {
  RMEM_REQUIRE(rings && verts && counts && workspace && rings_out && verts_out && counts_out,
               "rmem_polygon_simplify: null pointer (rings, verts, counts, workspace, rings_out, verts_out and counts_out are required)");
  RMEM_REQUIRE(capacities_ok(max_rings, max_verts), "rmem_polygon_simplify: max_rings and max_verts must be in 1..2^31-1");
  RMEM_REQUIRE(tolerance_16ths >= 0 && tolerance_16ths <= 1024, "rmem_polygon_simplify: tolerance_16ths must be in 0..1024");
  const Layout l = layout(max_rings, max_verts);
  RMEM_REQUIRE(workspace_bytes >= l.bytes, "rmem_polygon_simplify: the workspace is smaller than rmem_polygon_simplify_workspace_bytes says");
  RMEM_REQUIRE(((uintptr_t)workspace & 15u) == 0, "rmem_polygon_simplify: the workspace must be 16-byte aligned");
  char* ws = (char*)workspace;
  int* hdr = (int*)(ws + l.hdr);
  int* cnt = (int*)(ws + l.cnt);
  int* ibase = (int*)(ws + l.ibase);
  int* kc = (int*)(ws + l.kc);
  int* obase = (int*)(ws + l.obase);
  u64* mask = (u64*)(ws + l.mask);
  int2* state = (int2*)(ws + l.state);
  u64* key = (u64*)(ws + l.key);
  int* idx = (int*)(ws + l.idx);
  long long* bsum = (long long*)(ws + l.bsum);
  int* bbad = (int*)(ws + l.bbad);
  hipStream_t st = (hipStream_t)stream;
  const long long MR = max_rings, MV = max_verts;
  const int T = tolerance_16ths;
  const dim3 th(kThreads), one(1);
  const long long per_wave = (MR + kWaves - 1) / kWaves;
  const dim3 waves((unsigned)(per_wave < kMaxBlocks ? per_wave : kMaxBlocks));
  const long long chunks = (MR + kThreads - 1) / kThreads;
  const dim3 blocks((unsigned)(chunks < kLongBlocks ? chunks : kLongBlocks));
  const dim3 tiles((unsigned)(l.tiles < kMaxBlocks ? l.tiles : kMaxBlocks));
  hipLaunchKernelGGL(k_simp_count, tiles, th, 0, st, rings, counts, MR, MV, cnt, bsum, bbad);
  hipLaunchKernelGGL(k_simp_head, one, th, 0, st, counts, MR, MV, bsum, (const int*)bbad, hdr);
  hipLaunchKernelGGL(k_simp_apply, tiles, th, 0, st, (const int*)hdr, (const int*)cnt, (const long long*)bsum, ibase);
  hipLaunchKernelGGL(k_simp_short, waves, th, 0, st, rings, verts, hdr, (const int*)cnt, T, kc, mask);
  hipLaunchKernelGGL(k_simp_long, blocks, th, 0, st, rings, verts, hdr, (const int*)cnt, (const int*)ibase, T, MV, kc, state, key, idx);
  hipLaunchKernelGGL(k_simp_partial, tiles, th, 0, st, (const int*)hdr, (const int*)kc, bsum);
  hipLaunchKernelGGL(k_simp_bases, one, th, 0, st, (const int*)hdr, MV, bsum, counts_out);
  hipLaunchKernelGGL(k_simp_apply, tiles, th, 0, st, (const int*)hdr, (const int*)kc, (const long long*)bsum, obase);
  hipLaunchKernelGGL(k_simp_emit_short, waves, th, 0, st, rings, verts, (const int*)hdr, (const int*)cnt, (const int*)kc, (const int*)obase,
                     (const u64*)mask, MV, rings_out, verts_out);
  hipLaunchKernelGGL(k_simp_emit_long, blocks, th, 0, st, rings, verts, (const int*)hdr, (const int*)cnt, (const int*)ibase, (const int*)kc,
                     (const int*)obase, (const int2*)state, MV, rings_out, verts_out);
  return rmem_check_launch("rmem_polygon_simplify");
}
