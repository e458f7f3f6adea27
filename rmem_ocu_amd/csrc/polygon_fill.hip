// Annotation polygons filled into uint8 label stacks on the device (include/rmem.h, rmem_polygon_fill_labels): the even-odd rule
// sampled at pixel centres in exact integer arithmetic on 1/256-pixel fixed point.  Element-type agnostic: built once.
//
// Even-odd needs no ring structure: a shape is a bag of edges, and a pixel belongs to it iff an odd number of its edges cross the
// pixel's sample row at or left of the pixel's centre.  The host (polygons.py, PackedPolygons) quantises the vertices, lists the
// edges that cross at least one sample row of the frame, counts every edge's crossings and gives the exclusive prefix of those
// counts, so nothing is counted here and the grid of every launch is known without a readback.  Per shape the workspace holds a
// bit plane over the shape's box, bit i of a row = column x0 + i, rows padded to 32-bit words.
//
// One pass (a range of frames whose planes fit the workspace) is a memset of the planes and four launches, no host sync:
//   k_fill_check   one thread per shape: its table entry against the pass (frame, order, value, box, plane, the frame's range
//                  in the first-shape table); writes the shape's status word, 0 or RMEM_POLYFILL_ST_DESC.
//   k_fill_toggle  one thread per crossing, not per edge (a box over a whole frame has two edges of H crossings each): a bounded
//                  binary search in the crossing prefix for its edge, the row, the toggle column by the contract's int64 formula,
//                  clamped to the box, one integer XOR atomic on the plane word.  XOR commutes: the order of arrival cannot show.
//   k_fill_rows    one workgroup per shape, one thread per row of its box: the running XOR along the row turns toggles into
//                  membership -- shifts within a word, the parity so far carried across words.  A thread per row because the
//                  planes of annotation shapes are a few words wide (27 words at 854 columns at the most): a row is a short
//                  serial loop, and rows are what there are many of.
//   k_fill_paint   one thread per 16 bytes of an output row, cut at the 16-byte boundaries of the row's ADDRESS, so that every
//                  whole piece is one aligned 16-byte store wherever the stack starts and whatever W is; the ragged ends of a row
//                  are written byte by byte.  A thread walks its frame's shapes in listing order, skips those whose box misses
//                  its piece, reads the (at most two) plane words and overwrites the bytes whose bit is set: the later shape wins.
//                  Every byte of the pass's frames is stored, also in frames without shapes.
// Every index that comes from device memory is checked before it is used; a failed check sets a bit in the shape's status word
// instead of making the access, and a shape with a non-zero status paints nothing.  Every loop is bounded.
#include "label_wave.h"
#include "../../include/rmem.h"

namespace {
constexpr long long kMaxShapes = (long long)kMaxFrames * 255;
constexpr int kMaxEdges = 1 << 30;
constexpr long long kMaxCrossings = 2147483647LL;
constexpr long long kMaxPlaneWords = 1LL << 34;
constexpr int kMaxCoord = 1 << 28;      // 2^20 pixels in 1/256

__device__ __forceinline__ int words_of(int width) { return (width + 31) >> 5; }

// floor(a / b) for b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
  long long q = a / b;
  if (a % b < 0) --q;
  return q;
}

__global__ __launch_bounds__(kThreads) void k_fill_check(const RmemPolyShape* __restrict__ shapes, const int* __restrict__ frame_shape,
                                                         int nshapes, int H, int W, RmemPolyPass p, int* __restrict__ status) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.shapes) return;
  const int s = p.shape0 + i;
  const RmemPolyShape d = shapes[s];
  bool ok = d.frame >= p.frame0 && d.frame < p.frame0 + p.frames && d.value >= 1 && d.value <= 255;
  if (ok && i > 0) ok = shapes[s - 1].frame <= d.frame;               // shapes are listed frame by frame
  if (ok) {                                                           // the painter finds the shape through the frame's range
    const int a = frame_shape[d.frame], b = frame_shape[d.frame + 1];
    ok = a <= s && s < b && b <= nshapes;
  }
  if (ok) ok = d.x0 >= 0 && d.y0 >= 0 && d.x1 <= W && d.y1 <= H;
  if (ok && d.x0 < d.x1 && d.y0 < d.y1) {                             // a plane: inside the pass's part of the workspace
    const long long words = (long long)(d.y1 - d.y0) * words_of(d.x1 - d.x0);
    ok = d.plane >= p.plane0 && d.plane - p.plane0 <= p.plane_words - words;
  }
  status[s] = ok ? 0 : RMEM_POLYFILL_ST_DESC;
}

__global__ __launch_bounds__(kThreads) void k_fill_toggle(const int4* __restrict__ edge_xy, const int* __restrict__ edge_shape,
                                                          const int* __restrict__ edge_first, const RmemPolyShape* __restrict__ shapes,
                                                          int H, int W, RmemPolyPass p, unsigned* __restrict__ planes, int* status) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= p.crossings) return;
  const long long target = p.cross0 + t;
  int lo = 0, hi = p.edges - 1;                                       // the last edge of the pass whose first crossing is <= target
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (int)(((long long)lo + hi + 1) >> 1);
    if (edge_first[p.edge0 + mid] <= target) lo = mid;
    else hi = mid - 1;
  }
  const int e = p.edge0 + lo;
  int s = edge_shape[e];
  if (s < p.shape0 || s >= p.shape0 + p.shapes) {                     // named outside the pass: the bit goes to the nearest shape
    atomicOr(&status[s < p.shape0 ? p.shape0 : p.shape0 + p.shapes - 1], RMEM_POLYFILL_ST_DESC);
    return;
  }
  if (status[s] & RMEM_POLYFILL_ST_DESC) return;                      // its box and plane are not to be trusted
  const RmemPolyShape d = shapes[s];
  if (d.x0 >= d.x1 || d.y0 >= d.y1) return;                           // no plane
  int4 q = edge_xy[e];
  if (min(min(q.x, q.y), min(q.z, q.w)) < -kMaxCoord || max(max(q.x, q.y), max(q.z, q.w)) > kMaxCoord) {
    atomicOr(&status[s], RMEM_POLYFILL_ST_EDGE);
    return;
  }
  if (q.y > q.w) q = make_int4(q.z, q.w, q.x, q.y);                   // Y0 <= Y1
  const long long j = target - edge_first[e];
  const int ya = max(0, (q.y + 127) >> 8), yb = min(H, (q.w + 127) >> 8);      // rows with Y0 <= 256 y + 128 < Y1, in the frame
  if (j < 0 || target >= edge_first[e + 1] || j >= yb - ya) {         // also every horizontal edge: yb <= ya
    atomicOr(&status[s], RMEM_POLYFILL_ST_PREFIX);
    return;
  }
  const int y = ya + (int)j;
  if (y < d.y0 || y >= d.y1) {
    atomicOr(&status[s], RMEM_POLYFILL_ST_EDGE);
    return;
  }
  const long long dY = (long long)q.w - q.y, dX = (long long)q.z - q.x;      // dY > 0 here
  const long long num = (long long)q.x * dY + (256LL * y + 128 - q.y) * dX;
  long long c = -floor_div(128 * dY - num, 256 * dY);                 // the smallest c with (256 c + 128) dY >= num
  c = c < 0 ? 0 : (c > W ? W : c);
  if (c >= d.x1) return;                                              // toggles nothing inside the box
  const int rel = (int)(c < d.x0 ? 0 : c - d.x0);
  const long long word = d.plane - p.plane0 + (long long)(y - d.y0) * words_of(d.x1 - d.x0) + (rel >> 5);
  atomicXor(&planes[word], 1u << (rel & 31));
}

__global__ __launch_bounds__(kThreads) void k_fill_rows(const RmemPolyShape* __restrict__ shapes, RmemPolyPass p, unsigned* __restrict__ planes,
                                                        const int* __restrict__ status) {
  const int s = p.shape0 + blockIdx.x;
  if (status[s]) return;
  const RmemPolyShape d = shapes[s];
  if (d.x0 >= d.x1 || d.y0 >= d.y1) return;
  const int wpr = words_of(d.x1 - d.x0), rows = d.y1 - d.y0;
  for (int r = threadIdx.x; r < rows; r += kThreads) {
    unsigned* row = planes + (d.plane - p.plane0) + (long long)r * wpr;
    unsigned carry = 0;                                               // all ones when the toggles so far are odd
    for (int w = 0; w < wpr; ++w) {
      unsigned x = row[w];
      x ^= x << 1;
      x ^= x << 2;
      x ^= x << 4;
      x ^= x << 8;
      x ^= x << 16;
      x ^= carry;
      row[w] = x;
      carry = 0u - (x >> 31);
    }
  }
}

// the byte mask of a 4-bit mask: byte j = 0xff where bit j is set
__device__ __forceinline__ uint32_t bytes_of(unsigned b) { return (((b & 0xfu) * 0x00204081u) & 0x01010101u) * 0xffu; }

__global__ __launch_bounds__(kThreads) void k_fill_paint(const RmemPolyShape* __restrict__ shapes, const int* __restrict__ frame_shape,
                                                         const int* __restrict__ status, int H, int W, int pieces, RmemPolyPass p,
                                                         const unsigned* __restrict__ planes, unsigned char* __restrict__ labels) {
  const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (long long)H * pieces) return;
  const int f = p.frame0 + blockIdx.y, y = (int)(id / pieces), k = (int)(id - (long long)y * pieces);
  unsigned char* row = labels + ((size_t)f * H + y) * W;
  const int xs = k * 16 - (int)((uintptr_t)row & 15u);                // the piece holds columns xs .. xs + 15, cut at 16-byte addresses
  const int xa = max(xs, 0), xb = min(xs + 16, W);
  if (xa >= xb) return;
  uint32_t out[4] = {0, 0, 0, 0};
  int s0 = frame_shape[f], s1 = frame_shape[f + 1];
  s0 = max(s0, p.shape0);
  s1 = min(s1, p.shape0 + p.shapes);
  for (int s = s0; s < s1; ++s) {
    const RmemPolyShape d = shapes[s];
    if (d.frame != f || y < d.y0 || y >= d.y1 || xb <= d.x0 || xa >= d.x1 || status[s]) continue;
    const int wpr = words_of(d.x1 - d.x0);
    const unsigned* pr = planes + (d.plane - p.plane0) + (long long)(y - d.y0) * wpr;
    const int r0 = xs - d.x0, w = r0 >> 5;                            // bit r0 + i of the row is column xs + i; r0 may be negative
    const unsigned lo = (w >= 0 && w < wpr) ? pr[w] : 0u, hi = (w + 1 >= 0 && w + 1 < wpr) ? pr[w + 1] : 0u;
    unsigned bits = (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (r0 & 31)) & 0xffffu;
    const int a = max(xa, d.x0) - xs, b = min(xb, d.x1) - xs;         // the piece's bytes inside the box and the row: a < b
    bits &= (0xffffu >> (16 - b)) & (0xffffu << a);
    if (!bits) continue;
    const uint32_t v4 = (uint32_t)d.value * 0x01010101u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t m = bytes_of(bits >> (4 * g));
      out[g] = (out[g] & ~m) | (v4 & m);
    }
  }
  if (xs >= 0 && xs + 16 <= W) {
    *reinterpret_cast<uint4*>(row + xs) = make_uint4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (xs + i >= xa && xs + i < xb) row[xs + i] = (unsigned char)(out[i >> 2] >> (8 * (i & 3)));
  }
}

}  // namespace

extern "C" size_t rmem_polygon_fill_workspace_bytes(long long plane_words) {
  if (plane_words < 0 || plane_words > kMaxPlaneWords) return 0;
  return (((size_t)(plane_words > 0 ? plane_words : 1) * 4) + 15) & ~(size_t)15;
}

extern "C" int rmem_polygon_fill_labels(const int* edge_xy, const int* edge_shape, const int* edge_first, int nedges, const RmemPolyShape* shapes,
                                        int nshapes, const int* frame_shape, int frames, int H, int W, const RmemPolyPass* pass,
                                        void* workspace, size_t workspace_bytes, unsigned char* labels, int* status, void* stream) {
  RMEM_REQUIRE(edge_xy && edge_shape && edge_first && shapes && frame_shape && pass && workspace && labels && status,
               "rmem_polygon_fill_labels: null pointer (the edge columns, shapes, frame_shape, pass, workspace, labels and status are required)");
  RMEM_REQUIRE(frames >= 1 && frames <= kMaxFrames, "rmem_polygon_fill_labels: frames must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(frames, H, W), "rmem_polygon_fill_labels: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(nshapes >= 1 && nshapes <= kMaxShapes, "rmem_polygon_fill_labels: nshapes must be in 1..65535*255");
  RMEM_REQUIRE(nedges >= 0 && nedges <= kMaxEdges, "rmem_polygon_fill_labels: nedges must be in 0..2^30");
  const RmemPolyPass p = *pass;
  RMEM_REQUIRE(p.frame0 >= 0 && p.frames >= 1 && p.frames <= frames - p.frame0,
               "rmem_polygon_fill_labels: the pass's frames must be a non-empty range of the stack's");
  RMEM_REQUIRE(p.shape0 >= 0 && p.shapes >= 0 && p.shapes <= nshapes - p.shape0,
               "rmem_polygon_fill_labels: the pass's shapes must be a range of the table's");
  RMEM_REQUIRE(p.edge0 >= 0 && p.edges >= 0 && p.edges <= nedges - p.edge0, "rmem_polygon_fill_labels: the pass's edges must be a range of the list's");
  RMEM_REQUIRE(p.cross0 >= 0 && p.crossings >= 0 && p.crossings <= kMaxCrossings - p.cross0,
               "rmem_polygon_fill_labels: the pass's crossings must lie in 0..2^31-1");
  RMEM_REQUIRE(p.crossings == 0 || (p.edges >= 1 && p.shapes >= 1), "rmem_polygon_fill_labels: crossings need edges and shapes in the pass");
  RMEM_REQUIRE(p.plane0 >= 0 && p.plane_words >= 0 && p.plane_words <= kMaxPlaneWords,
               "rmem_polygon_fill_labels: the pass's plane words must be in 0..2^34");
  RMEM_REQUIRE(((uintptr_t)workspace & 15u) == 0, "rmem_polygon_fill_labels: the workspace must be 16-byte aligned");
  RMEM_REQUIRE(((uintptr_t)edge_xy & 15u) == 0, "rmem_polygon_fill_labels: edge_xy must be 16-byte aligned");
  RMEM_REQUIRE(workspace_bytes >= rmem_polygon_fill_workspace_bytes(p.plane_words),
               "rmem_polygon_fill_labels: the workspace is smaller than rmem_polygon_fill_workspace_bytes says");
  hipStream_t st = (hipStream_t)stream;
  unsigned* planes = (unsigned*)workspace;
  if (p.plane_words > 0 && hipMemsetAsync(planes, 0, (size_t)p.plane_words * 4, st) != hipSuccess) {
    rmem_set_error("rmem_polygon_fill_labels: hipMemsetAsync failed");
    return -1;
  }
  if (p.shapes > 0)
    hipLaunchKernelGGL(k_fill_check, dim3((unsigned)((p.shapes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, shapes, frame_shape, nshapes,
                       H, W, p, status);
  if (p.crossings > 0)
    hipLaunchKernelGGL(k_fill_toggle, dim3((unsigned)((p.crossings + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const int4*)edge_xy,
                       edge_shape, edge_first, shapes, H, W, p, planes, status);
  if (p.shapes > 0 && p.plane_words > 0)
    hipLaunchKernelGGL(k_fill_rows, dim3((unsigned)p.shapes), dim3(kThreads), 0, st, shapes, p, planes, (const int*)status);
  const int pieces = (W + 15) / 16 + 1;                               // H * pieces <= H * W / 16 + 2 H
  const long long threads = (long long)H * pieces;
  hipLaunchKernelGGL(k_fill_paint, dim3((unsigned)((threads + kThreads - 1) / kThreads), (unsigned)p.frames), dim3(kThreads), 0, st, shapes,
                     frame_shape, (const int*)status, H, W, pieces, p, (const unsigned*)planes, labels);
  return rmem_check_launch("rmem_polygon_fill_labels");
}
