// Label stacks traced into polygon rings (include/rmem.h, rmem_label_polygons): the outer contours and the holes of every object
// of every frame as closed rings of pixel corners, the format labelling tools and COCO `segmentation` lists take (polygons.py).
// Element-type agnostic (uint8 label stacks in, int32 rings and vertices out): built once.
//
// Every side of an object pixel whose neighbour does not hold the object's value is a directed unit edge with the object on its
// right; the successor rule of the header makes the edges of a frame a permutation whose cycles are the rings.  Nothing here
// follows a ring sequentially: the edges are compacted in (frame, edge id) order, every edge learns its ring's smallest edge and
// its distance to it by pointer doubling, and the rings are laid out by scans.  Separate launches, no kernel waits for or spins
// on another workgroup, every loop is bounded, integer arithmetic only, no host sync, everything on the caller's stream.
//
//   k_poly_walk<false>   one thread per unit = kRun pixels of a row (lanes = adjacent runs: a wave reads consecutive bytes of the
//                        rows y - 1, y, y + 1): the number of edges of its pixels, stored to the unit's own counter.
//   k_label_scan_units   one workgroup per frame: exclusive scan of its units' counts in place (unit order = edge id order), total
//                        (label_scan.h, which also holds the workgroup scan of the kernels below).
//   k_poly_base          one workgroup: scan over the frames' totals in 64 bits -> every frame's base; counts = (E, 0, 0, status).
//                        With E > max_edges the status says so and every later kernel returns at once.
//   k_poly_walk<true>    the same walk; edge ids go to base + running offset -- the compact array comes out sorted by (frame, edge
//                        id) -- and beside each its successor's edge id, from the pixel's 3 x 3 neighbourhood.
//   k_poly_link          successor edge id -> compact index: the successor's pixel names its unit, the unit's scanned count the
//                        at most 4 * kRun sorted ids to search.  Starts the doubling: (mn, dm, jump) = (next, 1, next).
//   k_poly_round         x ceil(log2(min(max_edges, 4 H W))), ping-pong: per edge the smallest compact index among the next 2^k
//                        edges of its walk, the distance to it, and the edge 2^k ahead.  j = jump[i]; if mn[j] < mn[i] take
//                        (mn[j], 2^k + dm[j]); jump[i] = jump[j].  Afterwards mn is the ring's start edge and dm the distance to
//                        it (the ring's length at the start itself: the nearer of equal candidates is kept).
//   k_poly_ringlen       per compact index: the ring's length at a start, 0 elsewhere, and the start flag.
//   k_poly_scan_*        (partial, sums, apply) exclusive scan of two int arrays of E entries at once, E + 1 results each: ring
//                        bases and ring numbers here, vertex numbers and area prefixes below.  Reduce, scan the block sums in
//                        one workgroup, re-scan: three launches, no look-back.
//   k_poly_order         order[ring base + rank] = edge, rank = (length - dm) % length: the edges ring by ring in walk order.
//   k_poly_corner        per position: 1 if the edge's heading differs from its predecessor's (the position before, the ring's
//                        last for its first), and the edge's shoelace term.  A ring's area2 is a difference of the scanned terms
//                        (unsigned arithmetic: the prefixes may wrap, the difference of at most 2^27 does not).
//   k_poly_emit          per position: a corner's vertex; from the ring's first position the ring's row; from position 0, R and V.
#include <limits.h>
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
constexpr int kRun = 8;                           // pixels of one row a thread walks: the walk unit
constexpr int kScanItems = 8;                     // entries per thread of the device-wide scans
constexpr int kScanTile = kThreads * kScanItems;

inline int units_x(int W) { return (W + kRun - 1) / kRun; }

struct Layout {
  size_t cnt, totals, fb, sums, eid, nxt, p0, p1, bytes;      // byte offsets into the workspace
  long long nb;                                               // blocks of one device-wide scan
};
Layout layout(int n, int H, int W, int M) {
  const size_t U = (size_t)H * units_x(W), M1 = (size_t)M + 1;
  Layout l;
  l.nb = (long long)((M1 + kScanTile - 1) / kScanTile);
  l.cnt = 0;
  l.totals = align16(l.cnt + (size_t)n * U * 4);
  l.fb = align16(l.totals + (size_t)n * 4);
  l.sums = align16(l.fb + ((size_t)n + 1) * 4);
  l.eid = align16(l.sums + (size_t)l.nb * 2 * 4);
  l.nxt = align16(l.eid + M1 * 4);
  l.p0 = align16(l.nxt + M1 * 4);
  l.p1 = align16(l.p0 + M1 * 16);
  l.bytes = align16(l.p1 + M1 * 16);
  return l;
}

// what every kernel after k_poly_base begins with: the number of edges, or -1 where they did not fit
__device__ __forceinline__ int edges_or_stop(const int* __restrict__ fb, int n, const int* counts) {
  if (counts[3] & RMEM_POLY_ST_CAPACITY) return -1;
  return fb[n];
}
// the frame of compact index i: the largest f with fb[f] <= i (n <= 65535: at most 16 steps)
__device__ __forceinline__ int frame_of(const int* __restrict__ fb, int n, int i) {
  int lo = 0, hi = n - 1;
  for (int it = 0; it < 17 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (fb[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------------------ the walk
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_poly_walk(const unsigned char* __restrict__ labels, int H, int W, int K, int conn8, int nxu, int U,
                                                        int M, int* __restrict__ cnt, const int* __restrict__ fb, const int* counts,
                                                        int* __restrict__ eid, int* __restrict__ nxt) {
  if (WRITE && (counts[3] & RMEM_POLY_ST_CAPACITY)) return;
  const int u = blockIdx.x * kThreads + threadIdx.x;
  if (u >= U) return;
  const int f = blockIdx.y;
  const int y = u / nxu, x0 = (u - y * nxu) * kRun;
  const unsigned char* L = labels + (size_t)f * H * W;
  int nb[3][kRun + 2];                                              // rows y - 1 .. y + 1, columns x0 - 1 .. x0 + kRun; 0 = not an object
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int yy = y + r - 1;
    const bool row_in = yy >= 0 && yy < H;
#pragma unroll
    for (int c = 0; c < kRun + 2; ++c) {
      const int xx = x0 + c - 1;
      int v = 0;
      if (row_in && xx >= 0 && xx < W) {
        v = L[(size_t)yy * W + xx];
        if (v > K) v = 0;
      }
      nb[r][c] = v;
    }
  }
  int* mine = cnt + (size_t)f * U + u;
  int at = WRITE ? fb[f] + *mine : 0, count = 0;
#pragma unroll
  for (int j = 1; j <= kRun; ++j) {
    const int v = nb[1][j];
    if (v == 0) continue;                                           // columns beyond W read 0 as well
    const int p = y * W + x0 + j - 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int across = s == 0 ? nb[0][j] : s == 1 ? nb[1][j + 1] : s == 2 ? nb[2][j] : nb[1][j - 1];
      if (across == v) continue;
      if (!WRITE) {
        ++count;
        continue;
      }
      // A: ahead on the right, B: ahead on the left of the edge's end vertex
      const int A = s == 0 ? nb[1][j + 1] : s == 1 ? nb[2][j] : s == 2 ? nb[1][j - 1] : nb[0][j];
      const int B = s == 0 ? nb[0][j + 1] : s == 1 ? nb[2][j + 1] : s == 2 ? nb[2][j - 1] : nb[0][j - 1];
      const int dA = s == 0 ? 1 : s == 1 ? W : s == 2 ? -1 : -W;
      const int dB = s == 0 ? 1 - W : s == 1 ? W + 1 : s == 2 ? W - 1 : -W - 1;
      const bool a = A == v, b = B == v;
      const bool left = conn8 ? b : (a && b), straight = !left && a;
      int next;
      if (left) next = (p + dB) * 4 + ((s + 3) & 3);
      else if (straight) next = (p + dA) * 4 + s;
      else next = p * 4 + ((s + 1) & 3);
      if (at >= 0 && at < M) {                                      // always, unless the labels changed between the two walks
        eid[at] = p * 4 + s;
        nxt[at] = next;
      }
      ++at;
    }
  }
  if (!WRITE) *mine = count;                                        // one owner: a plain store
}

__global__ __launch_bounds__(kThreads) void k_poly_base(const int* __restrict__ totals, int n, int M, int* __restrict__ fb, int* __restrict__ counts) {
  __shared__ long long sh[kWaves];
  long long carry = 0;
  for (int b = 0; b < n; b += kThreads) {
    const int i = b + threadIdx.x;
    const long long v = i < n ? totals[i] : 0;
    long long tot;
    const long long inc = block_incl_scan(v, sh, tot);
    if (i < n) fb[i] = (int)min(carry + inc - v, (long long)INT_MAX);
    carry += tot;
  }
  if (threadIdx.x == 0) {
    const int E = (int)min(carry, (long long)INT_MAX);
    fb[n] = E;
    counts[0] = E;
    counts[1] = 0;
    counts[2] = 0;
    counts[3] = carry > M ? RMEM_POLY_ST_CAPACITY : 0;
  }
}

// --------------------------------------------------------------------------------------------------- ring identity and rank
__global__ __launch_bounds__(kThreads) void k_poly_link(const int* __restrict__ fb, int n, int* counts, const int* __restrict__ cnt, int U,
                                                        int nxu, int W, int HW, const int* __restrict__ eid, const int* __restrict__ nxt,
                                                        int4* __restrict__ P) {
  const int E = edges_or_stop(fb, n, counts);
  const long long gi = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gi >= E) return;
  const int i = (int)gi;
  const int f = frame_of(fb, n, i);
  const int sid = nxt[i], q = sid >> 2;
  int found = -1;
  if ((unsigned)q < (unsigned)HW) {
    const int yq = q / W, u = yq * nxu + (q - yq * W) / kRun;
    const int* c = cnt + (size_t)f * U;
    int lo = fb[f] + c[u], hi = u + 1 < U ? fb[f] + c[u + 1] : fb[f + 1];
    if (lo < 0) lo = 0;
    if (hi > E) hi = E;
    for (int it = 0; it < 8 && lo < hi; ++it) {                     // at most 4 * kRun = 32 ids: 6 steps
      const int mid = (lo + hi) >> 1, e = eid[mid];
      if (e == sid) {
        found = mid;
        break;
      }
      if (e < sid) lo = mid + 1;
      else hi = mid;
    }
  }
  if (found < 0) {                                                  // never; a ring of its own keeps everything after in range
    atomicOr(counts + 3, RMEM_POLY_ST_LINK);
    found = i;
  }
  P[i] = make_int4(found, 1, found, 0);
}

__global__ __launch_bounds__(kThreads) void k_poly_round(const int* __restrict__ fb, int n, const int* counts, const int4* __restrict__ in,
                                                         int4* __restrict__ out, int step) {
  const int E = edges_or_stop(fb, n, counts);
  const long long gi = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gi >= E) return;
  int4 p = in[gi];
  const int4 q = in[p.z];                                           // p.z < E: k_poly_link wrote a compact index or i itself
  if (q.x < p.x) {
    p.x = q.x;
    p.y = step + q.y;
  }
  p.z = q.z;
  out[gi] = p;
}

__global__ __launch_bounds__(kThreads) void k_poly_ringlen(const int* __restrict__ fb, int n, const int* counts, const int4* __restrict__ P,
                                                           int* __restrict__ rb, int* __restrict__ ridx) {
  const int E = edges_or_stop(fb, n, counts);
  const long long gi = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gi >= E) return;
  const int4 p = P[gi];
  const bool start = p.x == (int)gi;
  rb[gi] = start ? p.y : 0;
  ridx[gi] = start;
}

// ------------------------------------------------------------------------------------- exclusive scan of two arrays, E + 1 results
__global__ __launch_bounds__(kThreads) void k_poly_scan_partial(const int* __restrict__ fb, int n, const int* counts, const int* __restrict__ a,
                                                                const int* __restrict__ b, unsigned* __restrict__ sums, long long nb) {
  __shared__ unsigned sh[kWaves];
  const int E = edges_or_stop(fb, n, counts);
  if (E < 0) return;
  const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  unsigned sa = 0, sb = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k < E) {
      sa += (unsigned)a[base + k];
      sb += (unsigned)b[base + k];
    }
  }
  unsigned ta, tb;
  block_incl_scan(sa, sh, ta);
  block_incl_scan(sb, sh, tb);
  if (threadIdx.x == 0) {
    sums[blockIdx.x] = ta;
    sums[nb + blockIdx.x] = tb;
  }
}

__global__ __launch_bounds__(kThreads) void k_poly_scan_sums(const int* __restrict__ fb, int n, const int* counts, unsigned* __restrict__ sums,
                                                             long long nb) {
  __shared__ unsigned sh[kWaves];
  if (edges_or_stop(fb, n, counts) < 0) return;
  unsigned* s = sums + nb * blockIdx.x;
  unsigned carry = 0;
  for (long long b = 0; b < nb; b += kThreads) {
    const long long i = b + threadIdx.x;
    const unsigned v = i < nb ? s[i] : 0;
    unsigned tot;
    const unsigned inc = block_incl_scan(v, sh, tot);
    if (i < nb) s[i] = carry + inc - v;
    carry += tot;
  }
}

// in place: a thread reads its entries before it writes them.  Entry E of both arrays receives the total.
__global__ __launch_bounds__(kThreads) void k_poly_scan_apply(const int* __restrict__ fb, int n, const int* counts, int* a, int* b,
                                                              const unsigned* __restrict__ sums, long long nb) {
  __shared__ unsigned sh[kWaves];
  const int E = edges_or_stop(fb, n, counts);
  if (E < 0) return;
  const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  unsigned va[kScanItems], vb[kScanItems], sa = 0, sb = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const bool in = base + k < E;
    va[k] = in ? (unsigned)a[base + k] : 0u;
    vb[k] = in ? (unsigned)b[base + k] : 0u;
    sa += va[k];
    sb += vb[k];
  }
  unsigned ta, tb;
  unsigned ea = block_incl_scan(sa, sh, ta) - sa + sums[blockIdx.x];
  unsigned eb = block_incl_scan(sb, sh, tb) - sb + sums[nb + blockIdx.x];
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k <= E) {
      a[base + k] = (int)ea;
      b[base + k] = (int)eb;
    }
    ea += va[k];
    eb += vb[k];
  }
}

// ------------------------------------------------------------------------------------------------------------- ring order
__global__ __launch_bounds__(kThreads) void k_poly_order(const int* __restrict__ fb, int n, int* counts, const int4* __restrict__ P,
                                                         const int* __restrict__ rb, int* __restrict__ order) {
  const int E = edges_or_stop(fb, n, counts);
  const long long gi = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gi >= E) return;
  const int4 p = P[gi];
  const int s = p.x;                                                // the ring's start: a compact index that the rounds copied
  const int len = P[s].y, d = p.y;
  const long long at = (long long)rb[s] + (d < len ? len - d : 0);
  if (len < 1 || d < 1 || d > len || at < 0 || at >= E) {           // never
    atomicOr(counts + 3, RMEM_POLY_ST_ORDER);
    return;
  }
  order[at] = (int)gi;
}

__global__ __launch_bounds__(kThreads) void k_poly_corner(const int* __restrict__ fb, int n, int* counts, const int4* __restrict__ P,
                                                          const int* __restrict__ rb, const int* __restrict__ order,
                                                          const int* __restrict__ eid, int W, int* __restrict__ corner, int* __restrict__ term) {
  const int E = edges_or_stop(fb, n, counts);
  const long long gp = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gp >= E) return;
  int c = 0, a = 0;
  const int i = order[gp];
  bool ok = (unsigned)i < (unsigned)E;                              // anything else: k_poly_order left the entry out (its status bit is set)
  if (ok) {
    const int s = P[i].x, len = P[s].y, b = rb[s];
    const long long before = gp == b ? (long long)b + len - 1 : gp - 1;
    ok = before >= 0 && before < E;
    if (ok) {
      const int j = order[before];
      ok = (unsigned)j < (unsigned)E;
      if (ok) {
        const int e = eid[i], side = e & 3, q = e >> 2;
        const int y = q / W, x = q - y * W;
        c = side != (eid[j] & 3);
        a = side == 0 ? -y : side == 1 ? x + 1 : side == 2 ? y + 1 : -x;   // x_from * y_to - x_to * y_from of the unit edge
      }
    }
  }
  if (!ok) atomicOr(counts + 3, RMEM_POLY_ST_ORDER);
  corner[gp] = c;
  term[gp] = a;
}

__global__ __launch_bounds__(kThreads) void k_poly_emit(const unsigned char* __restrict__ labels, const int* __restrict__ fb, int n, int* counts,
                                                        const int4* __restrict__ P, const int* __restrict__ rb, const int* __restrict__ ridx,
                                                        const int* __restrict__ order, const int* __restrict__ eid,
                                                        const int* __restrict__ cs, const int* __restrict__ as, int W, int HW, int M,
                                                        int* __restrict__ rings, int* __restrict__ verts) {
  const int E = edges_or_stop(fb, n, counts);
  const long long gp = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gp >= E) return;
  if (gp == 0) {
    counts[1] = ridx[E];
    counts[2] = cs[E];
  }
  const int i = order[gp];
  if ((unsigned)i >= (unsigned)E) return;                           // never: see k_poly_corner
  const int e = eid[i], side = e & 3, q = e >> 2;
  const int v0 = cs[gp];
  if (cs[gp + 1] != v0 && (unsigned)v0 < (unsigned)M) {             // the start corner of the edge
    const int y = q / W, x = q - y * W;
    verts[2 * (size_t)v0] = x + (side == 1 || side == 2);
    verts[2 * (size_t)v0 + 1] = y + (side == 2 || side == 3);
  }
  const int4 p = P[i];
  if (p.x != i || rb[i] != gp) return;                              // the ring's first position only
  const int len = p.y, r = ridx[i];
  if (gp + len > E || (unsigned)r > (unsigned)(M / 4)) return;      // never
  const int f = frame_of(fb, n, i);
  int* o = rings + 8 * (size_t)r;
  o[0] = f;
  o[1] = labels[(size_t)f * HW + q];
  o[2] = v0;
  o[3] = cs[gp + len] - v0;
  o[4] = (int)((unsigned)as[gp + len] - (unsigned)as[gp]);
  o[5] = e;
  o[6] = len;
  o[7] = 0;
}

}  // namespace

extern "C" int rmem_label_polygons_unit(void) { return kRun; }

extern "C" size_t rmem_label_polygons_workspace_bytes(int n, int H, int W, int max_edges) {
  if (!stack_geometry_ok(n, H, W) || max_edges < 4) return 0;
  return layout(n, H, W, max_edges).bytes;
}

extern "C" int rmem_label_polygons(const unsigned char* labels, int n, int H, int W, int num_objs, int connectivity, int max_edges,
                                   void* workspace, size_t workspace_bytes, int* rings, int* verts, int* counts, void* stream) {
  RMEM_REQUIRE(labels && workspace && rings && verts && counts,
               "rmem_label_polygons: null pointer (labels, workspace, rings, verts and counts are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_polygons: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_polygons: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(num_objs >= 1 && num_objs <= 255, "rmem_label_polygons: num_objs must be in 1..255");
  RMEM_REQUIRE(connectivity == 4 || connectivity == 8, "rmem_label_polygons: connectivity must be 4 or 8");
  RMEM_REQUIRE(max_edges >= 4, "rmem_label_polygons: max_edges must be at least 4");
  const Layout l = layout(n, H, W, max_edges);
  RMEM_REQUIRE(workspace_bytes >= l.bytes, "rmem_label_polygons: the workspace is smaller than rmem_label_polygons_workspace_bytes says");
  RMEM_REQUIRE(((uintptr_t)workspace & 15u) == 0, "rmem_label_polygons: the workspace must be 16-byte aligned");
  const int HW = H * W, M = max_edges, conn8 = connectivity == 8, nxu = units_x(W), U = H * nxu;
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + l.cnt);
  int* totals = (int*)(ws + l.totals);
  int* fb = (int*)(ws + l.fb);
  unsigned* sums = (unsigned*)(ws + l.sums);
  int* eid = (int*)(ws + l.eid);
  int* nxt = (int*)(ws + l.nxt);
  int4* pp[2] = {(int4*)(ws + l.p0), (int4*)(ws + l.p1)};
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(kThreads);
  const dim3 walk((unsigned)((U + kThreads - 1) / kThreads), (unsigned)n);
  const dim3 edges((unsigned)(((long long)M + kThreads - 1) / kThreads));
  const dim3 tiles((unsigned)l.nb);
  hipLaunchKernelGGL(k_poly_walk<false>, walk, th, 0, st, labels, H, W, num_objs, conn8, nxu, U, M, cnt, (const int*)nullptr, (const int*)nullptr,
                     (int*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(k_label_scan_units, dim3((unsigned)n), th, 0, st, cnt, U, totals);
  hipLaunchKernelGGL(k_poly_base, dim3(1), th, 0, st, (const int*)totals, n, M, fb, counts);
  hipLaunchKernelGGL(k_poly_walk<true>, walk, th, 0, st, labels, H, W, num_objs, conn8, nxu, U, M, cnt, (const int*)fb, (const int*)counts, eid, nxt);
  hipLaunchKernelGGL(k_poly_link, edges, th, 0, st, (const int*)fb, n, counts, (const int*)cnt, U, nxu, W, HW, (const int*)eid, (const int*)nxt, pp[0]);
  const long long longest = 4LL * HW < M ? 4LL * HW : M;             // no ring has more edges
  int rounds = 0;
  while ((1LL << rounds) < longest) ++rounds;
  for (int k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(k_poly_round, edges, th, 0, st, (const int*)fb, n, (const int*)counts, (const int4*)pp[k & 1], pp[(k + 1) & 1], 1 << k);
  const int4* P = pp[rounds & 1];
  int* spare = (int*)pp[(rounds + 1) & 1];                          // the other buffer: four arrays of M + 1 ints
  const size_t M1 = (size_t)M + 1;
  int *rb = spare, *ridx = spare + M1, *order = spare + 2 * M1, *cs = spare + 3 * M1, *as = nxt;   // nxt lives on in the jumps
  hipLaunchKernelGGL(k_poly_ringlen, edges, th, 0, st, (const int*)fb, n, (const int*)counts, P, rb, ridx);
  hipLaunchKernelGGL(k_poly_scan_partial, tiles, th, 0, st, (const int*)fb, n, (const int*)counts, (const int*)rb, (const int*)ridx, sums, l.nb);
  hipLaunchKernelGGL(k_poly_scan_sums, dim3(2), th, 0, st, (const int*)fb, n, (const int*)counts, sums, l.nb);
  hipLaunchKernelGGL(k_poly_scan_apply, tiles, th, 0, st, (const int*)fb, n, (const int*)counts, rb, ridx, (const unsigned*)sums, l.nb);
  hipLaunchKernelGGL(k_poly_order, edges, th, 0, st, (const int*)fb, n, counts, P, (const int*)rb, order);
  hipLaunchKernelGGL(k_poly_corner, edges, th, 0, st, (const int*)fb, n, counts, P, (const int*)rb, (const int*)order, (const int*)eid, W, cs, as);
  hipLaunchKernelGGL(k_poly_scan_partial, tiles, th, 0, st, (const int*)fb, n, (const int*)counts, (const int*)cs, (const int*)as, sums, l.nb);
  hipLaunchKernelGGL(k_poly_scan_sums, dim3(2), th, 0, st, (const int*)fb, n, (const int*)counts, sums, l.nb);
  hipLaunchKernelGGL(k_poly_scan_apply, tiles, th, 0, st, (const int*)fb, n, (const int*)counts, cs, as, (const unsigned*)sums, l.nb);
  hipLaunchKernelGGL(k_poly_emit, edges, th, 0, st, labels, (const int*)fb, n, counts, P, (const int*)rb, (const int*)ridx, (const int*)order,
                     (const int*)eid, (const int*)cs, (const int*)as, W, HW, M, rings, verts);
  return rmem_check_launch("rmem_label_polygons");
}
