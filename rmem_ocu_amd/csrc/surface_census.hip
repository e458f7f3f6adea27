// The surfaces of uint8 label stacks and the census of surface-to-surface distances (include/rmem.h: rmem_label_surface,
// rmem_surface_census; surface.py).  Integers only: no float decides anything, only integer atomics, so every
// result is bit-reproducible and independent of scheduling.  Element-type agnostic: built once.
//
//   k_label_surface   One thread per pixel: the pixel keeps its value if a 4-neighbour holds another value or lies outside the
//                     frame, else 0.  Byte loads and stores: the stacks may start anywhere, nothing outside the frame is read.
//   k_census_walk     Walks the key pixels (key in 1..num_objs) of one direction's stacks (blockIdx.z: 0 = a, 1 = b), four ways:
//                       pass 0      accumulates count, sum_fix, max and within[] of every (object, direction) in a table in LDS
//                                   (64-bit integer add and max), merged into the workspace with one global atomic per entry the
//                                   workgroup touched, and counts digit 0 (bits 29..20) of every sample in the histograms of its
//                                   own set and of the pooled set;
//                       pass 1, 2   counts digit 1 (bits 19..10) / digit 2 (bits 9..0) of the samples whose higher bits equal
//                                   the prefix its set has picked so far;
//                       pass 3      the smallest sample above `lo`, for the sets whose `hi` is not `lo` (an integer min).
//                     Sentinel samples join count and max only: a set holds sentinels only or none.
//   k_census_pick     One workgroup per (frame, object, set) after each digit pass: finds the bin that holds rank r_lo among the
//                     1024 counts (four per thread, a workgroup scan), appends it to the set's prefix, keeps the rank inside the
//                     bin and the number of samples below it, and clears the histogram for the next pass.  After digit 2 the
//                     prefix is `lo`, and `hi` is `lo` if more than r_hi samples are at or below it.
//   k_census_table    One thread per (frame, object): the three rows of the table.
//
// No kernel waits for another workgroup; every loop is bounded by the pixels of a frame, the objects or the bins.
#include <limits.h>
#include "label_wave.h"
#include "../../include/rmem.h"

namespace {
constexpr int kMaxSide = 16384;                    // label_sep.h: every real sample is below 2^30
constexpr int kSentinel = INT_MAX;
constexpr int kDigitBits = 10, kBins = 1 << kDigitBits, kDigits = 3;
constexpr int kAcc = 7;                            // count, sum_fix, max, within[4]
constexpr int kState = 8;                          // ints per set, below
constexpr int kMaxTol = 4;
static_assert(kDigits * kDigitBits == 30 && kBins == 4 * kThreads, "three digits cover a real sample; a thread owns four bins");
enum { S_ACTIVE = 0, S_PREFIX, S_RANK, S_BELOW, S_RHI, S_NEED, S_NEXT, S_PAD };

struct Tol {
  int t[kMaxTol];
};

__global__ __launch_bounds__(kThreads) void k_label_surface(const unsigned char* __restrict__ labels, int H, int W,
                                                            unsigned char* __restrict__ surface) {
  const int HW = H * W;
  const unsigned char* L = labels + (size_t)blockIdx.y * HW;
  unsigned char* S = surface + (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < HW; p += gridDim.x * kThreads) {
    const int y = p / W, x = p - y * W, v = L[p];
    const bool edge = x == 0 || L[p - 1] != v || x == W - 1 || L[p + 1] != v || y == 0 || L[p - W] != v || y == H - 1 || L[p + W] != v;
    S[p] = (unsigned char)(edge ? v : 0);
  }
}

// floor(sqrt(d2 * 2^32)), d2 < 2^30: the double root is a seed, 64-bit integer compares decide
__device__ __forceinline__ unsigned long long root_fix(int d2) {
  const unsigned long long v = (unsigned long long)d2 << 32;
  unsigned long long r = (unsigned long long)sqrt((double)v);
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (r * r > v) --r;
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// hist[idx] += the number of lanes with `on` and this idx: the lanes of a wave that share a bin add once (on dense surfaces most
// do).  Called by whole waves; at most 64 turns, every turn retires its leader.
__device__ __forceinline__ void wave_count(unsigned* hist, int idx, bool on, int lane) {
  unsigned long long todo = __ballot(on);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int want = __shfl(idx, lead, 64);
    const unsigned long long same = __ballot(on && idx == want);
    if (lane == lead) atomicAdd(hist + idx, (unsigned)__popcll(same));
    todo &= ~same;
  }
}

// acc  [n][K][2][kAcc] int64, state [n][K][3][kState] int32, hist [n][K][3][kBins] uint32
__global__ __launch_bounds__(kThreads) void k_census_walk(const int* __restrict__ samples_a, const unsigned char* __restrict__ keys_a,
                                                          const int* __restrict__ samples_b, const unsigned char* __restrict__ keys_b, int HW,
                                                          int K, Tol tol, int num_tol, int pass, unsigned long long* __restrict__ acc,
                                                          int* __restrict__ state, unsigned* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* tab = (unsigned long long*)smem;               // [K][kAcc], pass 0 only
  const int t = threadIdx.x, f = blockIdx.y, dir = blockIdx.z;
  const int* D = (dir ? samples_b : samples_a) + (size_t)f * HW;
  const unsigned char* Kv = (dir ? keys_b : keys_a) + (size_t)f * HW;
  if (pass == 0) {
    for (int i = t; i < K * kAcc; i += kThreads) tab[i] = 0ull;
    __syncthreads();
  }
  const int shift = (kDigits - 1 - pass) * kDigitBits;               // of this pass' digit (passes 0..2)
  const int* fstate = state + (size_t)f * K * 3 * kState;
  unsigned* fhist = hist + (size_t)f * K * 3 * kBins;
  for (int p0 = blockIdx.x * kThreads; p0 < HW; p0 += gridDim.x * kThreads) {        // the same trips in every lane of a wave
    const int p = p0 + t;
    const int k = p < HW ? Kv[p] : 0;
    const bool keyed = k >= 1 && k <= K;
    const int d2 = keyed ? D[p] : kSentinel;
    if (pass == 0 && keyed) {
      unsigned long long* row = tab + (k - 1) * kAcc;
      atomicAdd(row + 0, 1ull);
      // entries only grow: a stale read can only let through a max that changes nothing
      if ((unsigned long long)d2 > __hip_atomic_load(row + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(row + 2, (unsigned long long)d2);
      if (d2 != kSentinel) {
        atomicAdd(row + 1, root_fix(d2));
        for (int j = 0; j < num_tol; ++j)
          if (d2 <= tol.t[j]) atomicAdd(row + 3 + j, 1ull);
      }
    }
    const bool real = keyed && (unsigned)d2 < 1u << (kDigits * kDigitBits);          // not the sentinel; nothing else indexes a bin
    for (int j = 0; j < 2; ++j) {                                    // the own set, then the pooled one
      const int set = (k - 1) * 3 + (j ? 2 : dir);                   // of this frame; looked up only where `real`
      const int* st = fstate + set * kState;
      if (pass == 0) {
        wave_count(fhist, set * kBins + (d2 >> shift), real, t & 63);
      } else if (pass < kDigits) {
        const bool on = real && st[S_ACTIVE] && (d2 >> (shift + kDigitBits)) == st[S_PREFIX];
        wave_count(fhist, set * kBins + ((d2 >> shift) & (kBins - 1)), on, t & 63);
      } else if (real && st[S_NEED] && d2 > st[S_PREFIX]) {
        int* next = state + ((size_t)f * K * 3 + set) * kState + S_NEXT;
        // entries only shrink: a stale read can only let through a min that changes nothing
        if (d2 < __hip_atomic_load(next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(next, d2);
      }
    }
  }
  if (pass == 0) {
    __syncthreads();
    for (int i = t; i < K * kAcc; i += kThreads) {
      const unsigned long long v = tab[i];
      if (!v) continue;
      unsigned long long* dst = acc + (((size_t)f * K + i / kAcc) * 2 + dir) * kAcc + i % kAcc;
      if (i % kAcc == 2) atomicMax(dst, v); else atomicAdd(dst, v);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_census_pick(const unsigned long long* __restrict__ acc, int* __restrict__ state,
                                                          unsigned* __restrict__ hist, int q, int pass) {
  __shared__ unsigned part[kThreads];
  const int t = threadIdx.x, s = blockIdx.x % 3;
  const size_t obj = blockIdx.x / 3;
  int* st = state + (obj * 3 + s) * kState;
  if (pass == 0) {                                                   // the ranks, from the set's count
    const unsigned long long* a0 = acc + obj * 2 * kAcc;
    const unsigned long long* a1 = a0 + kAcc;
    const long long m = (s != 1 ? (long long)a0[0] : 0) + (s != 0 ? (long long)a1[0] : 0);
    const unsigned long long mx = max(s != 1 ? a0[2] : 0ull, s != 0 ? a1[2] : 0ull);
    const bool active = m > 0 && mx != (unsigned long long)kSentinel;
    if (!active) {                                                   // empty, or sentinels only: the histogram is all zero
      if (t == 0) st[S_ACTIVE] = 0, st[S_NEED] = 0;
      return;
    }
    if (t == 0) {
      const long long r_lo = (m - 1) * q / 10000;
      st[S_ACTIVE] = 1;
      st[S_PREFIX] = 0;
      st[S_RANK] = (int)r_lo;
      st[S_BELOW] = 0;
      st[S_RHI] = (int)min(r_lo + 1, m - 1);
      st[S_NEED] = 0;
      st[S_NEXT] = kSentinel;
    }
    __syncthreads();
  } else if (!st[S_ACTIVE]) {
    return;                                                          // the same in every thread: written by an earlier launch
  }
  unsigned* h = hist + (obj * 3 + s) * kBins + 4 * t;
  const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
  h[0] = h[1] = h[2] = h[3] = 0u;                                    // clean for the next pass and the next call
  part[t] = c0 + c1 + c2 + c3;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {                           // inclusive scan of the 256 partial sums
    const unsigned v = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const unsigned rank = (unsigned)st[S_RANK], before = t ? part[t - 1] : 0u;
  __syncthreads();                                                   // every thread has read the rank
  if (rank >= before && rank < part[t]) {                            // exactly one thread: the counts add up to more than rank
    unsigned cum = before;
    int bin = 4 * t;
    if (rank >= cum + c0) { cum += c0; ++bin;
      if (rank >= cum + c1) { cum += c1; ++bin;
        if (rank >= cum + c2) { cum += c2; ++bin; } } }
    const unsigned in_bin = bin == 4 * t ? c0 : bin == 4 * t + 1 ? c1 : bin == 4 * t + 2 ? c2 : c3;
    st[S_PREFIX] = (st[S_PREFIX] << kDigitBits) | bin;
    st[S_RANK] = (int)(rank - cum);
    st[S_BELOW] += (int)cum;
    if (pass == kDigits - 1) st[S_NEED] = (unsigned)st[S_BELOW] + in_bin > (unsigned)st[S_RHI] ? 0 : 1;
  }
}

__global__ __launch_bounds__(kThreads) void k_census_table(const unsigned long long* __restrict__ acc, const int* __restrict__ state,
                                                           long long objs, long long* __restrict__ table) {
  const long long obj = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (obj >= objs) return;
  const unsigned long long* a = acc + obj * 2 * kAcc;
  for (int s = 0; s < 3; ++s) {
    long long row[kAcc];
#pragma unroll
    for (int j = 0; j < kAcc; ++j) {
      const long long v0 = s != 1 ? (long long)a[j] : 0, v1 = s != 0 ? (long long)a[kAcc + j] : 0;
      row[j] = j == 2 ? max(v0, v1) : v0 + v1;
    }
    const int* st = state + (obj * 3 + s) * kState;
    long long* out = table + (obj * 3 + s) * 9;
    long long lo = -1, hi = -1;
    if (row[0] > 0 && row[2] == kSentinel) {
      lo = hi = kSentinel;
    } else if (row[0] > 0) {
      lo = st[S_PREFIX];
      hi = st[S_NEED] ? st[S_NEXT] : lo;
    }
    out[0] = row[0];
    out[1] = row[1];
    out[2] = row[0] > 0 ? row[2] : -1;
    out[3] = lo;
    out[4] = hi;
#pragma unroll
    for (int j = 0; j < kMaxTol; ++j) out[5 + j] = row[3 + j];
  }
}

constexpr long long kPerObject = 2 * kAcc * 8 + 3 * kState * 4 + 3 * kBins * 4;      // acc, state, hist: 12496 bytes
}  // namespace

extern "C" int rmem_label_surface(const unsigned char* labels, int n, int H, int W, unsigned char* surface, void* stream) {
  RMEM_REQUIRE(labels && surface, "rmem_label_surface: null pointer (labels and surface are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_label_surface: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_label_surface: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(H <= kMaxSide && W <= kMaxSide, "rmem_label_surface: H and W must be at most 16384");
  hipLaunchKernelGGL(k_label_surface, dim3(blocks_per_frame(16L * H * W, n), n), dim3(kThreads), 0, (hipStream_t)stream, labels, H, W, surface);
  return rmem_check_launch("rmem_label_surface");
}

extern "C" long long rmem_surface_census_workspace_bytes(int n, int num_objs) {
  if (n < 1 || n > kMaxFrames || num_objs < 1 || num_objs > 255) return 0;
  return (long long)n * num_objs * kPerObject;
}

extern "C" int rmem_surface_census(const int* samples_a, const unsigned char* keys_a, const int* samples_b, const unsigned char* keys_b, int n,
                                   int H, int W, int num_objs, const int* tol2, int num_tol, int q, long long* table, void* workspace,
                                   long long workspace_bytes, void* stream) {
  RMEM_REQUIRE(samples_a && keys_a && samples_b && keys_b && table && workspace,
               "rmem_surface_census: null pointer (samples, keys, table and workspace are required)");
  RMEM_REQUIRE(n >= 1 && n <= kMaxFrames, "rmem_surface_census: n must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(n, H, W), "rmem_surface_census: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(H <= kMaxSide && W <= kMaxSide, "rmem_surface_census: H and W must be at most 16384");
  RMEM_REQUIRE(num_objs >= 1 && num_objs <= 255, "rmem_surface_census: num_objs must be in 1..255");
  RMEM_REQUIRE(num_tol >= 0 && num_tol <= kMaxTol, "rmem_surface_census: num_tol must be in 0..4");
  RMEM_REQUIRE(num_tol == 0 || tol2, "rmem_surface_census: null pointer (tol2 is required with num_tol > 0)");
  RMEM_REQUIRE(q >= 0 && q <= 10000, "rmem_surface_census: q must be in 0..10000 (hundredths of a percent)");
  Tol tol = {{0, 0, 0, 0}};
  for (int j = 0; j < num_tol; ++j) {
    RMEM_REQUIRE(tol2[j] >= 0 && tol2[j] < (1 << 30), "rmem_surface_census: every tol2 must be in 0..2^30 - 1");
    tol.t[j] = tol2[j];
  }
  RMEM_REQUIRE(workspace_bytes >= rmem_surface_census_workspace_bytes(n, num_objs),
               "rmem_surface_census: workspace too small (rmem_surface_census_workspace_bytes)");
  RMEM_REQUIRE(((uintptr_t)workspace & 7u) == 0, "rmem_surface_census: workspace must be 8-byte aligned");
  const long long objs = (long long)n * num_objs;
  unsigned long long* acc = (unsigned long long*)workspace;
  int* state = (int*)(acc + objs * 2 * kAcc);
  unsigned* hist = (unsigned*)(state + objs * 3 * kState);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, (size_t)(objs * kPerObject), s) != hipSuccess) {
    rmem_set_error("rmem_surface_census: clearing the workspace failed");
    return -1;
  }
  const int HW = H * W;
  const dim3 walk(blocks_per_frame(16L * HW, 2 * n), n, 2);
  for (int pass = 0; pass <= kDigits; ++pass) {
    hipLaunchKernelGGL(k_census_walk, walk, dim3(kThreads), pass == 0 ? (size_t)num_objs * kAcc * 8 : 0, s, samples_a, keys_a, samples_b,
                       keys_b, HW, num_objs, tol, num_tol, pass, acc, state, hist);
    if (pass < kDigits) hipLaunchKernelGGL(k_census_pick, dim3((unsigned)(objs * 3)), dim3(kThreads), 0, s, acc, state, hist, q, pass);
  }
  hipLaunchKernelGGL(k_census_table, dim3((unsigned)((objs + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, acc, state, objs, table);
  return rmem_check_launch("rmem_surface_census");
}
