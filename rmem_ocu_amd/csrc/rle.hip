// COCO run-length masks on the device, both directions (include/rmem.h, rmem_rle_encode_labels / rmem_rle_decode_labels).
// Element-type agnostic (uint8 label stacks and bytes in and out): built once.
//
// A mask is read column-major, position j = x * H + y.  For a label map, the run boundaries of all objects together are the
// label transitions in that order with label[-1] := 0: a transition a -> b at j is a boundary of object a (a != 0) and of object
// b (b != 0), and object k's counts are the differences of its sorted boundary positions, closed by H * W.  One walk over the
// labels therefore serves every object, and the walk is done twice: once to count, once to write.
//
// Writing (8 launches, no host sync):
//   k_rle_walk<false>  one thread per (column x, chunk of kChunkRows rows): the labels of its piece, row by row (lanes = adjacent
//                      columns, so a wave's loads are 64 consecutive bytes), compared with the pixel before in column-major order.
//                      Every boundary adds 1 to cnt[frame][id][x * NC + chunk]; that counter has exactly one owner thread, so the
//                      no-return integer atomic is only a cheap read-modify-write: its order cannot show.
//   k_label_scan_units one workgroup per (frame, id): exclusive scan of its units in place (unit order = position order), its total
//                      (label_scan.h, which also holds the workgroup scan every kernel below uses).
//   k_rle_base         one workgroup per frame: where each id's positions start in the frame's position array (<= 2 H W entries).
//   k_rle_walk<true>   the same walk; a boundary is stored at base + the unit's running offset: positions come out sorted.
//   k_rle_sizes        one workgroup per (frame, id): counts from positions, the delta (count i minus count i - 2 for i > 2), the
//                      number of 5-bit characters of each, their sum = the string's size.
//   k_rle_offsets      one workgroup: int64 exclusive scan of the sizes -> offsets, and the status word (capacity).
//   k_rle_emit         one workgroup per (frame, id): the same lengths, a scan per tile of 256 counts, the characters.  Nothing is
//                      written when the total exceeds the capacity.
// An id absent from a frame costs a scan over zeros and a one-count string.
//
// Reading (4 launches, no host sync):
//   k_rle_parse        one workgroup per string: descriptor check; per character its validity, whether it ends a count (0x20 clear)
//                      and the count it ends, assembled by looking back at most 5 characters; a scan of the end flags gives the
//                      count's index.  Then the un-delta (two interleaved prefix sums, even and odd indices) and the prefix sum to
//                      run ends, in 64 bits so that no crafted string wraps into a valid one; validation.  Count i of a string is
//                      kept at workspace int [string offset + i]: a string has no more counts than bytes.  Last, per column
//                      the run that holds its top pixel (W binary searches): the painter then looks at one column's runs only.
//   k_rle_ranges       the first and last string of every frame (strings are listed frame by frame), by integer max.
//   k_rle_paint        one thread per four consecutive pixels of a column, lanes = adjacent columns (a store instruction writes 64
//                      consecutive bytes of a row): the frame's strings from the last listed to the first; in each whose set
//                      range covers these positions, a binary search among the column's runs; the first hit wins.
#include "label_scan.h"
#include "../../include/rmem.h"

namespace {
constexpr int kChunkRows = 128;       // rows of one column a thread walks
constexpr int kLoadRows = 16;         // loads in flight per thread
constexpr long long kMaxStrings = (long long)kMaxFrames * 255;

inline int chunks_of(int H) { return (H + kChunkRows - 1) / kChunkRows; }

// ---------------------------------------------------------------------------------------------------------------- writing
struct EncodeLayout {
  size_t cnt, totals, base, sizes, pos, bytes;      // byte offsets into the workspace
};
EncodeLayout encode_layout(int frames, int H, int W, int K) {
  const size_t U = (size_t)W * chunks_of(H), fk = (size_t)frames * K;
  EncodeLayout l;
  l.cnt = 0;
  l.totals = align16(l.cnt + fk * U * 4);
  l.base = align16(l.totals + fk * 4);
  l.sizes = align16(l.base + fk * 4);
  l.pos = align16(l.sizes + fk * 4);
  l.bytes = align16(l.pos + (size_t)frames * 2 * H * W * 4);
  return l;
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_rle_walk(const unsigned char* __restrict__ labels, int H, int W, int K, int NC, int nxb,
                                                       int* cnt, const int* __restrict__ base, int* __restrict__ pos) {
  const int chunk = blockIdx.x / nxb, xb = blockIdx.x - chunk * nxb;
  const int x = xb * kThreads + threadIdx.x;
  if (x >= W) return;
  const int f = blockIdx.y;
  const size_t HW = (size_t)H * W, U = (size_t)W * NC;
  const unsigned char* L = labels + f * HW;
  const int y0 = chunk * kChunkRows, y1 = min(H, y0 + kChunkRows);
  int prev = 0;                                                     // the pixel before (x, y0) in column-major order
  if (y0 > 0) prev = L[(size_t)(y0 - 1) * W + x];
  else if (x > 0) prev = L[(size_t)(H - 1) * W + x - 1];
  if (prev > K) prev = 0;
  int* c = cnt + (size_t)f * K * U + (size_t)x * NC + chunk;        // + (id - 1) * U: this thread's counter of id
  int* p = WRITE ? pos + (size_t)f * 2 * HW : nullptr;
  const int* b = WRITE ? base + (size_t)f * K : nullptr;
  auto boundary = [&](int id, int j) {
    int* ci = c + (size_t)(id - 1) * U;
    if (!WRITE) {
      atomicAdd(ci, 1);
    } else {
      const int slot = *ci;                                         // one owner: a plain read-modify-write
      *ci = slot + 1;
      const size_t at = (size_t)b[id - 1] + slot;
      if (at < 2 * HW) p[at] = j;                                   // always, unless the labels changed between the two walks
    }
  };
  for (int y = y0; y < y1; y += kLoadRows) {
    int v[kLoadRows];
#pragma unroll
    for (int r = 0; r < kLoadRows; ++r) v[r] = y + r < y1 ? L[(size_t)(y + r) * W + x] : 0;
#pragma unroll
    for (int r = 0; r < kLoadRows; ++r) {
      if (y + r < y1) {
        const int cur = v[r] > K ? 0 : v[r];
        if (cur != prev) {
          const int j = x * H + y + r;
          if (prev) boundary(prev, j);
          if (cur) boundary(cur, j);
          prev = cur;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_rle_base(const int* __restrict__ totals, int K, int* __restrict__ base) {
  __shared__ int sh[kWaves];
  const int t = threadIdx.x;
  const size_t at = (size_t)blockIdx.x * K + t;
  const int v = t < K ? totals[at] : 0;
  int tot;
  const int inc = block_incl_scan(v, sh, tot);
  if (t < K) base[at] = inc - v;
}

// count i of the mask whose n sorted boundary positions are p (N = H * W): n + 1 counts
__device__ __forceinline__ int rle_count(const int* __restrict__ p, int n, int N, int i) {
  return (i < n ? p[i] : N) - (i > 0 ? p[i - 1] : 0);
}
__device__ __forceinline__ int rle_delta(const int* __restrict__ p, int n, int N, int i) {
  return rle_count(p, n, N, i) - (i > 2 ? rle_count(p, n, N, i - 2) : 0);
}
__device__ __forceinline__ int rle_nchars(int x) {
  int n = 0;
  bool more;
  do {
    const int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    ++n;
  } while (more);
  return n;
}

__global__ __launch_bounds__(kThreads) void k_rle_sizes(const int* __restrict__ pos, const int* __restrict__ totals, const int* __restrict__ base,
                                                        int K, int HW, int* __restrict__ sizes) {
  __shared__ int sh[kWaves];
  const int fk = blockIdx.x, f = fk / K;
  const int n = totals[fk];
  const int* p = pos + (size_t)f * 2 * HW + base[fk];
  int sum = 0;
  for (int i = threadIdx.x; i <= n; i += kThreads) sum += rle_nchars(rle_delta(p, n, HW, i));
  int tot;
  block_incl_scan(sum, sh, tot);
  if (threadIdx.x == 0) sizes[fk] = tot;
}

__global__ __launch_bounds__(kThreads) void k_rle_offsets(const int* __restrict__ sizes, long long S, long long capacity,
                                                          long long* __restrict__ offsets, int* __restrict__ status) {
  __shared__ long long sh[kWaves];
  long long carry = 0;
  for (long long b = 0; b < S; b += kThreads) {
    const long long i = b + threadIdx.x;
    const long long v = i < S ? sizes[i] : 0;
    long long tot;
    const long long inc = block_incl_scan(v, sh, tot);
    if (i < S) offsets[i] = carry + inc - v;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    offsets[S] = carry;
    status[0] = carry > capacity ? RMEM_RLE_ST_CAPACITY : 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_rle_emit(const int* __restrict__ pos, const int* __restrict__ totals, const int* __restrict__ base,
                                                       int K, int HW, const long long* __restrict__ offsets, long long S, long long capacity,
                                                       unsigned char* __restrict__ out) {
  __shared__ int sh[kWaves];
  if (offsets[S] > capacity) return;
  const int fk = blockIdx.x, f = fk / K;
  const int n = totals[fk];
  const int* p = pos + (size_t)f * 2 * HW + base[fk];
  unsigned char* o = out + offsets[fk];
  const long long room = offsets[fk + 1] - offsets[fk];
  long long carry = 0;
  for (int b = 0; b <= n; b += kThreads) {
    const int i = b + threadIdx.x;
    int x = 0, len = 0;
    if (i <= n) {
      x = rle_delta(p, n, HW, i);
      len = rle_nchars(x);
    }
    int tot;
    const int inc = block_incl_scan(len, sh, tot);
    long long at = carry + inc - len;
    if (at + len <= room) {                                         // always: the sizes came from the same positions
      for (int k = 0; k < len; ++k) {
        int c = x & 0x1f;
        x >>= 5;
        if (k + 1 < len) c |= 0x20;
        o[at + k] = (unsigned char)(c + 48);
      }
    }
    carry += tot;
  }
}

// ---------------------------------------------------------------------------------------------------------------- reading
struct DecodeLayout {
  size_t ends, meta, range, cols, bytes;
};
DecodeLayout decode_layout(long long nstrings, long long total_bytes, int frames, int W) {
  DecodeLayout l;
  l.ends = 0;
  l.meta = align16(l.ends + (size_t)(total_bytes > 0 ? total_bytes : 1) * 4);
  l.range = align16(l.meta + (size_t)nstrings * 16);
  l.cols = align16(l.range + (size_t)frames * 2 * 4);
  l.bytes = align16(l.cols + (size_t)nstrings * W * 4);
  return l;
}

// the run that holds position j: the smallest i in lo..hi with q[i] > j (run i is [q[i - 1], q[i]); the caller knows q[hi] > j)
__device__ __forceinline__ int run_of(const int* __restrict__ q, int lo, int hi, int j) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid] > j) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// meta[s] = (number of counts, first set position, end of the last set run, 0); number 0 = the string paints nothing
__global__ __launch_bounds__(kThreads) void k_rle_parse(const unsigned char* __restrict__ bits, long long total_bytes,
                                                        const RmemRleDesc* __restrict__ descs, int frames, int H, int W, int* __restrict__ ends,
                                                        int4* __restrict__ meta, int* __restrict__ cols, int* __restrict__ status) {
  __shared__ int shi[kWaves];
  __shared__ long long shl[kWaves];
  __shared__ int sh_err;
  const int s = blockIdx.x, t = threadIdx.x, HW = H * W;
  const RmemRleDesc d = descs[s];
  int st = 0;
  if (d.frame < 0 || d.frame >= frames || d.value < 1 || d.value > 255 || d.offset < 0 || d.length < 0 || d.offset > total_bytes - d.length) {
    st = RMEM_RLE_ST_DESC;
  } else if (s > 0) {
    const int pf = descs[s - 1].frame;                              // strings are listed frame by frame
    if (pf >= 0 && pf < frames && pf > d.frame) st = RMEM_RLE_ST_DESC;
  }
  if (st) {                                                         // uniform over the workgroup
    if (t == 0) {
      status[s] = st;
      meta[s] = make_int4(0, 0, 0, 0);
    }
    return;
  }
  const unsigned char* str = bits + d.offset;
  int* p = ends + d.offset;
  const int len = d.length;
  if (t == 0) sh_err = 0;
  int err = 0, m = 0;
  for (int b = 0; b < len; b += kThreads) {
    const int i = b + t;
    int end = 0, x = 0;
    if (i < len) {
      const int c = (int)str[i] - 48;
      if (c < 0 || c > 63) {
        err |= RMEM_RLE_ST_CHAR;
      } else {
        int run = 0;                                                // continuation characters right before this one, at most 6
        while (run < 6 && i - run - 1 >= 0 && (((int)str[i - run - 1] - 48) & 0x20)) ++run;
        if (run == 6) err |= RMEM_RLE_ST_LONG;                      // the seventh (or a later) character of one count
        if (!(c & 0x20)) {
          end = 1;
          if (run < 6) {
            unsigned u = 0;
            for (int k = 0; k <= run; ++k) u |= (unsigned)(((int)str[i - run + k] - 48) & 0x1f) << (5 * k);
            if (c & 0x10) u |= ~0u << (5 * (run + 1));              // at most 30 bits are taken
            x = (int)u;
          }
        } else if (i == len - 1) {
          err |= RMEM_RLE_ST_TRUNCATED;
        }
      }
    }
    int tot;
    const int inc = block_incl_scan(end, shi, tot);
    if (end) p[m + inc - 1] = x;                                    // at most i ends before character i: inside the string's ints
    m += tot;
  }
  __syncthreads();
  if (err) atomicOr(&sh_err, err);
  __syncthreads();
  if (sh_err) {
    if (t == 0) {
      status[s] = sh_err;
      meta[s] = make_int4(0, 0, 0, 0);
    }
    return;
  }
  long long carry_e = 0, carry_o = 0, carry_p = 0;
  for (int b = 0; b < m; b += kThreads) {
    const int i = b + t;
    const long long x = i < m ? p[i] : 0;
    long long te, to, tp;
    const long long ie = block_incl_scan<long long>((i >= 2 && !(i & 1)) ? x : 0, shl, te);
    const long long io = block_incl_scan<long long>((i & 1) ? x : 0, shl, to);
    long long c = i == 0 ? x : ((i & 1) ? carry_o + io : carry_e + ie);
    if (i >= m) c = 0;
    if (c < 0) err |= RMEM_RLE_ST_NEGATIVE;
    const long long ip = block_incl_scan<long long>(c, shl, tp);
    if (i < m) p[i] = (int)(carry_p + ip);                          // exact whenever the string turns out valid
    carry_e += te;
    carry_o += to;
    carry_p += tp;
  }
  if (carry_p != HW) err |= RMEM_RLE_ST_SUM;
  __syncthreads();
  if (err) atomicOr(&sh_err, err);
  __syncthreads();
  if (t == 0) {
    const int e = sh_err;
    status[s] = e;
    if (e) meta[s] = make_int4(0, 0, 0, 0);
    else meta[s] = make_int4(m, p[0], (m & 1) ? (m >= 3 ? p[m - 2] : 0) : HW, 0);
  }
  if (sh_err) return;
  int* cs = cols + (size_t)s * W;                                   // the run that holds the top pixel of every column
  for (int x = t; x < W; x += kThreads) cs[x] = run_of(p, 0, m - 1, x * H);
}

// range[2f] = nstrings - (the first string of frame f), range[2f + 1] = its last string + 1; both zeroed before: an empty range
// for a frame without strings.  Integer max only: the order of arrival cannot show, whatever the listing looks like.
__global__ __launch_bounds__(kThreads) void k_rle_ranges(const RmemRleDesc* __restrict__ descs, int nstrings, int frames, int* __restrict__ range) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= nstrings) return;
  const int f = descs[s].frame;
  if (f < 0 || f >= frames) return;
  if (s == 0 || descs[s - 1].frame != f) atomicMax(&range[2 * f], nstrings - s);
  if (s == nstrings - 1 || descs[s + 1].frame != f) atomicMax(&range[2 * f + 1], s + 1);
}

// One thread per four pixels of one column (rows 4g .. 4g + 3 of column x; the 64 lanes of a wave are adjacent columns, so
// every store instruction writes 64 consecutive bytes of a row).  The four positions are consecutive and nearly always lie in
// one run: one search among the column's runs for the first, a step forward where a run ends in between.
__global__ __launch_bounds__(kThreads) void k_rle_paint(const RmemRleDesc* __restrict__ descs, const int* __restrict__ ends,
                                                        const int4* __restrict__ meta, const int* __restrict__ range,
                                                        const int* __restrict__ cols, int nstrings, int H, int W, int nxb,
                                                        unsigned char* __restrict__ labels) {
  const int f = blockIdx.y;
  const int by = blockIdx.x / nxb, bx = blockIdx.x - by * nxb;
  const int x = bx * 64 + (threadIdx.x & 63), y0 = (by * kWaves + (threadIdx.x >> 6)) * 4;
  if (x >= W || y0 >= H) return;
  const int npx = min(4, H - y0), j0 = x * H + y0;
  unsigned todo = (1u << npx) - 1u, out = 0;
  const int first = nstrings - range[2 * f];
  for (int s = range[2 * f + 1] - 1; s >= first && todo; --s) {
    const int4 mt = meta[s];
    if (mt.x == 0 || j0 + npx <= mt.y || j0 >= mt.z) continue;       // not painted, or no set pixel among these positions
    const RmemRleDesc d = descs[s];
    if (d.frame != f) continue;
    const int* q = ends + d.offset;                                 // run i is [q[i - 1], q[i]); q[m - 1] = H * W
    const int* cs = cols + (size_t)s * W;
    // between the run of this column's top pixel and the run of the next column's, whose end is beyond every j of this column
    int r = run_of(q, cs[x], x + 1 < W ? cs[x + 1] : mt.x - 1, j0);
    int e = q[r];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < npx) {
        while (e <= j0 + i) e = q[++r];                             // ends at q[m - 1] = H * W > j at the latest
        if ((r & 1) && ((todo >> i) & 1u)) {
          out |= (unsigned)d.value << (8 * i);
          todo &= ~(1u << i);
        }
      }
    }
  }
  unsigned char* o = labels + (size_t)f * H * W + (size_t)y0 * W + x;
  for (int i = 0; i < npx; ++i) o[(size_t)i * W] = (unsigned char)(out >> (8 * i));
}

}  // namespace

extern "C" size_t rmem_rle_workspace_bytes(int frames, int H, int W, int num_ids) {
  if (!stack_geometry_ok(frames, H, W) || num_ids < 1 || num_ids > 255) return 0;
  return encode_layout(frames, H, W, num_ids).bytes;
}

extern "C" int rmem_rle_encode_labels(const unsigned char* labels, int frames, int H, int W, int num_ids, void* workspace, unsigned char* out,
                                      long long capacity, long long* offsets, int* status, void* stream) {
  RMEM_REQUIRE(labels && workspace && out && offsets && status,
               "rmem_rle_encode_labels: null pointer (labels, workspace, out, offsets and status are required)");
  RMEM_REQUIRE(frames >= 1 && frames <= kMaxFrames, "rmem_rle_encode_labels: frames must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(frames, H, W), "rmem_rle_encode_labels: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(num_ids >= 1 && num_ids <= 255, "rmem_rle_encode_labels: num_ids must be in 1..255");
  RMEM_REQUIRE(capacity >= 0, "rmem_rle_encode_labels: capacity must not be negative");
  RMEM_REQUIRE(((uintptr_t)workspace & 15u) == 0, "rmem_rle_encode_labels: the workspace must be 16-byte aligned");
  const int K = num_ids, NC = chunks_of(H), HW = H * W;
  const long long U = (long long)W * NC, S = (long long)frames * K;       // U <= H * W / 128 + W
  const EncodeLayout l = encode_layout(frames, H, W, K);
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + l.cnt);
  int* totals = (int*)(ws + l.totals);
  int* base = (int*)(ws + l.base);
  int* sizes = (int*)(ws + l.sizes);
  int* pos = (int*)(ws + l.pos);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(cnt, 0, l.totals - l.cnt, st) != hipSuccess) {
    rmem_set_error("rmem_rle_encode_labels: hipMemsetAsync failed");
    return -1;
  }
  const int nxb = (W + kThreads - 1) / kThreads;
  const dim3 walk((unsigned)(nxb * NC), (unsigned)frames);
  hipLaunchKernelGGL(k_rle_walk<false>, walk, dim3(kThreads), 0, st, labels, H, W, K, NC, nxb, cnt, (const int*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(k_label_scan_units, dim3((unsigned)S), dim3(kThreads), 0, st, cnt, (int)U, totals);
  hipLaunchKernelGGL(k_rle_base, dim3((unsigned)frames), dim3(kThreads), 0, st, totals, K, base);
  hipLaunchKernelGGL(k_rle_walk<true>, walk, dim3(kThreads), 0, st, labels, H, W, K, NC, nxb, cnt, (const int*)base, pos);
  hipLaunchKernelGGL(k_rle_sizes, dim3((unsigned)S), dim3(kThreads), 0, st, pos, totals, base, K, HW, sizes);
  hipLaunchKernelGGL(k_rle_offsets, dim3(1), dim3(kThreads), 0, st, sizes, S, capacity, offsets, status);
  hipLaunchKernelGGL(k_rle_emit, dim3((unsigned)S), dim3(kThreads), 0, st, pos, totals, base, K, HW, offsets, S, capacity, out);
  return rmem_check_launch("rmem_rle_encode_labels");
}

extern "C" size_t rmem_rle_decode_workspace_bytes(long long nstrings, long long total_bytes, int frames, int W) {
  if (nstrings < 1 || nstrings > kMaxStrings || total_bytes < 0 || total_bytes > INT32_MAX || frames < 1 || frames > kMaxFrames || W < 1 ||
      W > kMaxPixels)
    return 0;
  return decode_layout(nstrings, total_bytes, frames, W).bytes;
}

extern "C" int rmem_rle_decode_labels(const unsigned char* bits, long long total_bytes, const RmemRleDesc* descs, int nstrings, int frames, int H,
                                      int W, void* workspace, unsigned char* labels, int* status, void* stream) {
  RMEM_REQUIRE(bits && descs && workspace && labels && status,
               "rmem_rle_decode_labels: null pointer (bits, descs, workspace, labels and status are required)");
  RMEM_REQUIRE(total_bytes >= 0 && total_bytes <= INT32_MAX, "rmem_rle_decode_labels: total_bytes must be in 0..2^31-1");
  RMEM_REQUIRE(nstrings >= 1 && nstrings <= kMaxStrings, "rmem_rle_decode_labels: nstrings must be in 1..65535*255");
  RMEM_REQUIRE(frames >= 1 && frames <= kMaxFrames, "rmem_rle_decode_labels: frames must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(frames, H, W), "rmem_rle_decode_labels: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(((uintptr_t)workspace & 15u) == 0, "rmem_rle_decode_labels: the workspace must be 16-byte aligned");
  const DecodeLayout l = decode_layout(nstrings, total_bytes, frames, W);
  char* ws = (char*)workspace;
  int* ends = (int*)(ws + l.ends);
  int4* meta = (int4*)(ws + l.meta);
  int* range = (int*)(ws + l.range);
  int* cols = (int*)(ws + l.cols);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(range, 0, (size_t)frames * 2 * 4, st) != hipSuccess) {
    rmem_set_error("rmem_rle_decode_labels: hipMemsetAsync failed");
    return -1;
  }
  hipLaunchKernelGGL(k_rle_parse, dim3((unsigned)nstrings), dim3(kThreads), 0, st, bits, total_bytes, descs, frames, H, W, ends, meta, cols, status);
  hipLaunchKernelGGL(k_rle_ranges, dim3((unsigned)((nstrings + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, descs, nstrings, frames, range);
  const int nxb = (W + 63) / 64, nyb = (H + 4 * kWaves - 1) / (4 * kWaves);      // nxb * nyb <= H * W / 1024 + H / 16 + W / 64 + 1
  hipLaunchKernelGGL(k_rle_paint, dim3((unsigned)(nxb * nyb), (unsigned)frames), dim3(kThreads), 0, st, descs, (const int*)ends,
                     (const int4*)meta, (const int*)range, (const int*)cols, nstrings, H, W, nxb, labels);
  return rmem_check_launch("rmem_rle_decode_labels");
}
