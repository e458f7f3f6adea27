// Strokes drawn into uint8 label stacks on the device (include/rmem.h, rmem_stroke_draw_labels): scribbles, clicks and polylines
// with a round brush of any radius or as 8-connected hairlines, in exact integer arithmetic on 1/256-pixel fixed point, pixel
// centres at integers.  Element-type agnostic: built once.
//
// The host (strokes.py, PackedStrokes) quantises the points, cuts every stroke into segments, orients the hairline ones, counts
// every segment's work items and gives the exclusive prefix of those counts, so the grid of every launch is known without a
// readback.  Per STROKED frame of a pass the workspace holds an int32 owner map [H][W]: the largest (index within the frame) + 1
// of the strokes that cover the pixel, 0 for none.  The later stroke wins, and the maximum commutes: the order of arrival cannot show.
//
// One pass (a range of frames whose owner maps fit the workspace) is a memset of the maps and four launches, no host sync:
//   k_stroke_check     one thread per stroke: its table entry against the pass (frame, order, the frame's range in the first-stroke
//                      table, value, radius, box, slot); writes the stroke's status word, 0 or RMEM_STROKE_ST_DESC.
//   k_stroke_segments  one thread per segment: the stroke it names, its coordinates, a hairline's orientation, its box inside the
//                      stroke's, its work items against the prefix; ORs into the status word.  A maximum cannot be taken back, so
//                      everything that can fail is looked at here, before the first atomic.
//   k_stroke_cover     one lane per work item, found by a bounded binary search in the prefix.  Round brush: one ROW of the
//                      segment's box, not one segment -- a segment over the whole frame must not serialise.  The columns of the row
//                      are narrowed first to what the capsule can reach there: the part of the segment within R of the row in y,
//                      its extent in x, R more on either side (a conservative integer bound; a corner-to-corner diagonal costs
//                      O(R) tests per row, not W), and the contract's exact test decides every pixel.  Hairline: one endpoint or one
//                      major-axis sample.  A covered pixel is one integer atomicMax on its owner word.
//   k_stroke_paint     one thread per 16 bytes of an output row, cut at the 16-byte boundaries of the row's ADDRESS, as k_fill_paint
//                      does.  Where the owner is not zero the byte is the owning stroke's value; otherwise 0, or the byte that was
//                      there in `over` mode, where a piece without any owner is not stored at all and frames without strokes are
//                      not touched.
// Every index that comes from device memory is checked before it is used; every loop is bounded.
#include "label_wave.h"
#include "../../include/rmem.h"

namespace {
constexpr int kMaxStrokes = 1 << 30;
constexpr int kMaxSegs = 1 << 30;
constexpr long long kMaxItems = 2147483647LL;
constexpr int kMaxCoord = 1 << 28;      // 2^20 pixels in 1/256
constexpr int kMaxRadius = 1 << 16;     // 256 pixels in 1/256

// floor(a / b) for b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
  long long q = a / b;
  if (a % b < 0) --q;
  return q;
}

// the box of a segment clipped to the frame, and what its work items are counted from
struct SegGeom {
  int x0, y0, x1, y1;   // columns x0..x1-1, rows y0..y1-1
  int items;            // 0 when the box is empty
  int ka;               // hairline: the major index of the first sample
  bool xmajor;          // hairline: the major axis is x
};

__device__ __forceinline__ SegGeom seg_geom(int4 q, int R, int H, int W) {
  SegGeom g;
  const int lox = min(q.x, q.z), hix = max(q.x, q.z), loy = min(q.y, q.w), hiy = max(q.y, q.w);
  const int below = R > 0 ? 255 - R : 128, above = R > 0 ? R : 128;   // ceil((lo - R) / 256) .. floor((hi + R) / 256), or half up
  g.x0 = max(0, (lox + below) >> 8);
  g.x1 = min(W, ((hix + above) >> 8) + 1);
  g.y0 = max(0, (loy + below) >> 8);
  g.y1 = min(H, ((hiy + above) >> 8) + 1);
  g.ka = 0;
  g.xmajor = true;
  if (g.x0 >= g.x1 || g.y0 >= g.y1) {
    g.items = 0;
    return g;
  }
  if (R > 0) {
    g.items = g.y1 - g.y0;
    return g;
  }
  const int dx = q.z - q.x, dy = q.w - q.y;
  g.xmajor = abs(dx) >= abs(dy);
  const int am = g.xmajor ? lox : loy, bm = g.xmajor ? hix : hiy, top = g.xmajor ? W : H;   // whichever way it runs
  g.ka = max(0, (am + 255) >> 8);
  const int kb = min(top - 1, bm >> 8);
  g.items = 2 + ((dx | dy) != 0 && kb >= g.ka ? kb - g.ka + 1 : 0);
  return g;
}

__global__ __launch_bounds__(kThreads) void k_stroke_check(const RmemStroke* __restrict__ strokes, const int* __restrict__ frame_stroke,
                                                           const int* __restrict__ stroked, int nstrokes, int H, int W, RmemStrokePass p,
                                                           int* __restrict__ status) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.strokes) return;
  const int s = p.stroke0 + i;
  const RmemStroke d = strokes[s];
  bool ok = d.frame >= p.frame0 && d.frame < p.frame0 + p.frames && d.value >= 0 && d.value <= 255 && d.radius >= 0 && d.radius <= kMaxRadius;
  if (ok && i > 0) ok = strokes[s - 1].frame <= d.frame;               // strokes are listed frame by frame
  if (ok) {                                                           // the painter finds the stroke through the frame's range
    const int a = frame_stroke[d.frame], b = frame_stroke[d.frame + 1];
    ok = a <= s && s < b && b <= nstrokes;
  }
  if (ok) ok = d.x0 >= 0 && d.y0 >= 0 && d.x0 <= d.x1 && d.y0 <= d.y1 && d.x1 <= W && d.y1 <= H;
  if (ok) ok = d.slot >= p.slot0 && d.slot < p.slot0 + p.slots;       // an owner map of the pass, and the frame's own
  if (ok) ok = stroked[d.slot] == d.frame;
  status[s] = ok ? 0 : RMEM_STROKE_ST_DESC;
}

__global__ __launch_bounds__(kThreads) void k_stroke_segments(const int4* __restrict__ seg_xy, const int* __restrict__ seg_stroke,
                                                              const int* __restrict__ seg_first, const RmemStroke* __restrict__ strokes,
                                                              int H, int W, RmemStrokePass p, int* status) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.segs) return;
  const int e = p.seg0 + i;
  const int s = seg_stroke[e];
  if (s < p.stroke0 || s >= p.stroke0 + p.strokes) {                  // named outside the pass: the bit goes to the nearest stroke
    atomicOr(&status[s < p.stroke0 ? p.stroke0 : p.stroke0 + p.strokes - 1], RMEM_STROKE_ST_DESC);
    return;
  }
  const RmemStroke d = strokes[s];
  if (d.radius < 0 || d.radius > kMaxRadius) return;                  // k_stroke_check has said so
  const int4 q = seg_xy[e];
  int bits = 0;
  if (min(min(q.x, q.y), min(q.z, q.w)) < -kMaxCoord || max(max(q.x, q.y), max(q.z, q.w)) > kMaxCoord) {
    atomicOr(&status[s], RMEM_STROKE_ST_SEGMENT);
    return;
  }
  const SegGeom g = seg_geom(q, d.radius, H, W);
  if (d.radius == 0 && (q.x != q.z || q.y != q.w) && (g.xmajor ? q.z - q.x : q.w - q.y) <= 0) bits |= RMEM_STROKE_ST_SEGMENT;
  if (g.items > 0 && (g.x0 < d.x0 || g.y0 < d.y0 || g.x1 > d.x1 || g.y1 > d.y1)) bits |= RMEM_STROKE_ST_SEGMENT;
  const long long first = seg_first[e], next = seg_first[e + 1];
  if (next - first != g.items) bits |= RMEM_STROKE_ST_PREFIX;
  if (i == 0 && first != p.item0) bits |= RMEM_STROKE_ST_PREFIX;
  if (i == p.segs - 1 && next != p.item0 + p.items) bits |= RMEM_STROKE_ST_PREFIX;
  if (bits) atomicOr(&status[s], bits);
}

// the contract's test of the pixel centre (px, py), in 1/256, against the segment q under R2 = R^2, L = d.d
__device__ __forceinline__ bool covered(long long px, long long py, int4 q, long long dx, long long dy, unsigned long long R2, long long L) {
  const long long wx = px - q.x, wy = py - q.y;
  const long long t = wx * dx + wy * dy;
  if (t <= 0) return (unsigned long long)(wx * wx + wy * wy) <= R2;
  if (t >= L) {
    const long long ux = px - q.z, uy = py - q.w;
    return (unsigned long long)(ux * ux + uy * uy) <= R2;
  }
  const long long c = wx * dy - wy * dx;
  const unsigned long long a = (unsigned long long)(c < 0 ? -c : c);
  const unsigned long long lhi = __umul64hi(a, a), llo = a * a;
  const unsigned long long rhi = __umul64hi(R2, (unsigned long long)L), rlo = R2 * (unsigned long long)L;
  return lhi < rhi || (lhi == rhi && llo <= rlo);
}

__global__ __launch_bounds__(kThreads) void k_stroke_cover(const int4* __restrict__ seg_xy, const int* __restrict__ seg_stroke,
                                                           const int* __restrict__ seg_first, const RmemStroke* __restrict__ strokes,
                                                           const int* __restrict__ frame_stroke, const int* __restrict__ status, int H, int W,
                                                           RmemStrokePass p, int* __restrict__ owner) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= p.items) return;
  const long long target = p.item0 + t;
  int lo = 0, hi = p.segs - 1;                                        // the last segment of the pass whose first item is <= target
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (int)(((long long)lo + hi + 1) >> 1);
    if (seg_first[p.seg0 + mid] <= target) lo = mid;
    else hi = mid - 1;
  }
  const int e = p.seg0 + lo;
  const int s = seg_stroke[e];
  if (s < p.stroke0 || s >= p.stroke0 + p.strokes || status[s]) return;      // a stroke with a status draws nothing
  const RmemStroke d = strokes[s];                                    // checked: frame, frame_stroke's range, radius, slot
  const int4 q = seg_xy[e];
  const SegGeom g = seg_geom(q, d.radius, H, W);
  const long long j = target - seg_first[e];
  if (j < 0 || j >= g.items) return;                                  // only with a prefix whose ends are not the pass's
  const int mark = s - frame_stroke[d.frame] + 1;
  int* map = owner + (size_t)(d.slot - p.slot0) * H * W;
  const long long dx = (long long)q.z - q.x, dy = (long long)q.w - q.y;
  if (d.radius > 0) {
    const int y = g.y0 + (int)j;
    const long long R = d.radius, py = 256LL * y;
    long long xmin = min(q.x, q.z), xmax = max(q.x, q.z);
    if (dy != 0) {                                                    // the part of the segment within R of the row, in y: its x extent
      const long long ay = dy > 0 ? q.y : q.w, ax = dy > 0 ? q.x : q.z, ex = dy > 0 ? dx : -dx, ey = dy > 0 ? dy : -dy;
      const long long n0 = min(max(py - R - ay, 0LL), ey), n1 = min(max(py + R - ay, 0LL), ey);
      const long long a0 = ex * n0, a1 = ex * n1;
      xmin = ax + min(floor_div(a0, ey), floor_div(a1, ey));
      xmax = ax - min(floor_div(-a0, ey), floor_div(-a1, ey));
    }
    const int xa = (int)max((long long)g.x0, (xmin - R + 255) >> 8), xb = (int)min((long long)g.x1, ((xmax + R) >> 8) + 1);
    const unsigned long long R2 = (unsigned long long)(R * R);
    const long long L = dx * dx + dy * dy;
    int* row = map + (size_t)y * W;
    for (int x = xa; x < xb; ++x)
      if (covered(256LL * x, py, q, dx, dy, R2, L)) atomicMax(&row[x], mark);
    return;
  }
  int x, y;
  if (j < 2) {                                                        // an endpoint, rounded half up per axis
    x = ((j == 0 ? q.x : q.z) + 128) >> 8;
    y = ((j == 0 ? q.y : q.w) + 128) >> 8;
  } else {                                                            // a major-axis sample: dM > 0 here
    const long long k = g.ka + (j - 2);
    const long long am = g.xmajor ? q.x : q.y, an = g.xmajor ? q.y : q.x, dM = g.xmajor ? dx : dy, dn = g.xmajor ? dy : dx;
    const long long N = an * dM + (256 * k - am) * dn;
    const long long n = floor_div(N + 128 * dM, 256 * dM);
    x = (int)(g.xmajor ? k : n);
    y = (int)(g.xmajor ? n : k);
  }
  if (x >= g.x0 && x < g.x1 && y >= g.y0 && y < g.y1) atomicMax(&map[(size_t)y * W + x], mark);
}

__global__ __launch_bounds__(kThreads) void k_stroke_paint(const RmemStroke* __restrict__ strokes, const int* __restrict__ frame_stroke,
                                                           const int* __restrict__ stroked, const int* __restrict__ status, int H, int W,
                                                           int pieces, RmemStrokePass p, const int* __restrict__ owner, int over,
                                                           unsigned char* __restrict__ labels) {
  const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (long long)H * pieces) return;
  const int f = p.frame0 + blockIdx.y, y = (int)(id / pieces), k = (int)(id - (long long)y * pieces);
  int lo = 0, hi = p.slots - 1;                                       // the frame's owner map: the slot whose entry in `stroked` is f
  for (int it = 0; it < 20 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if (stroked[p.slot0 + mid] < f) lo = mid + 1;
    else hi = mid;
  }
  const bool has = p.slots > 0 && stroked[p.slot0 + lo] == f;
  if (!has && over) return;
  unsigned char* row = labels + ((size_t)f * H + y) * W;
  const int xs = k * 16 - (int)((uintptr_t)row & 15u);                // the piece holds columns xs .. xs + 15, cut at 16-byte addresses
  const int xa = max(xs, 0), xb = min(xs + 16, W);
  if (xa >= xb) return;
  const bool whole = xs >= 0 && xs + 16 <= W;
  uint32_t out[4] = {0, 0, 0, 0}, mask[4] = {0, 0, 0, 0};
  if (has) {
    int s0 = frame_stroke[f], s1 = frame_stroke[f + 1];
    const int base = s0;
    s0 = max(s0, p.stroke0);
    s1 = min(s1, p.stroke0 + p.strokes);
    const int* orow = owner + ((size_t)lo * H + y) * W;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int x = xs + i;
      if (x < xa || x >= xb) continue;
      const int o = orow[x];
      if (o <= 0) continue;
      const long long s = (long long)base + o - 1;
      if (s < s0 || s >= s1 || status[s]) continue;
      const RmemStroke d = strokes[s];
      if (d.frame != f) continue;
      out[i >> 2] |= (uint32_t)(d.value & 0xff) << (8 * (i & 3));
      mask[i >> 2] |= 0xffu << (8 * (i & 3));
    }
  }
  if (over) {
    if (!(mask[0] | mask[1] | mask[2] | mask[3])) return;
    if (whole) {
      const uint4 was = *reinterpret_cast<const uint4*>(row + xs);
      *reinterpret_cast<uint4*>(row + xs) = make_uint4((was.x & ~mask[0]) | out[0], (was.y & ~mask[1]) | out[1], (was.z & ~mask[2]) | out[2],
                                                      (was.w & ~mask[3]) | out[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((mask[i >> 2] >> (8 * (i & 3))) & 1u) row[xs + i] = (unsigned char)(out[i >> 2] >> (8 * (i & 3)));
    }
    return;
  }
  if (whole) {
    *reinterpret_cast<uint4*>(row + xs) = make_uint4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (xs + i >= xa && xs + i < xb) row[xs + i] = (unsigned char)(out[i >> 2] >> (8 * (i & 3)));
  }
}

}  // namespace

extern "C" size_t rmem_stroke_workspace_bytes(int stroked_frames, int H, int W) {
  if (stroked_frames < 0 || stroked_frames > kMaxFrames || H < 1 || W < 1 || (long)H * W > kMaxPixels) return 0;
  const size_t words = (size_t)stroked_frames * (size_t)H * (size_t)W;
  return (((words > 0 ? words : 1) * 4) + 15) & ~(size_t)15;
}

extern "C" int rmem_stroke_draw_labels(const int* seg_xy, const int* seg_stroke, const int* seg_first, int nsegs, const RmemStroke* strokes,
                                       int nstrokes, const int* frame_stroke, const int* stroked, int nstroked, int frames, int H, int W,
                                       const RmemStrokePass* pass, void* workspace, size_t workspace_bytes, unsigned char* labels, int over,
                                       int* status, void* stream) {
  RMEM_REQUIRE(seg_xy && seg_stroke && seg_first && strokes && frame_stroke && stroked && pass && workspace && labels && status,
               "rmem_stroke_draw_labels: null pointer (the segment columns, strokes, frame_stroke, stroked, pass, workspace, labels and status are "
               "required)");
  RMEM_REQUIRE(frames >= 1 && frames <= kMaxFrames, "rmem_stroke_draw_labels: frames must be in 1..65535");
  RMEM_REQUIRE(stack_geometry_ok(frames, H, W), "rmem_stroke_draw_labels: H and W must be positive, H * W at most 2^26");
  RMEM_REQUIRE(nstrokes >= 1 && nstrokes <= kMaxStrokes, "rmem_stroke_draw_labels: nstrokes must be in 1..2^30");
  RMEM_REQUIRE(nsegs >= 0 && nsegs <= kMaxSegs, "rmem_stroke_draw_labels: nsegs must be in 0..2^30");
  RMEM_REQUIRE(nstroked >= 1 && nstroked <= frames, "rmem_stroke_draw_labels: nstroked must be in 1..frames");
  const RmemStrokePass p = *pass;
  RMEM_REQUIRE(p.frame0 >= 0 && p.frames >= 1 && p.frames <= frames - p.frame0,
               "rmem_stroke_draw_labels: the pass's frames must be a non-empty range of the stack's");
  RMEM_REQUIRE(p.stroke0 >= 0 && p.strokes >= 0 && p.strokes <= nstrokes - p.stroke0,
               "rmem_stroke_draw_labels: the pass's strokes must be a range of the table's");
  RMEM_REQUIRE(p.seg0 >= 0 && p.segs >= 0 && p.segs <= nsegs - p.seg0, "rmem_stroke_draw_labels: the pass's segments must be a range of the list's");
  RMEM_REQUIRE(p.slot0 >= 0 && p.slots >= 0 && p.slots <= nstroked - p.slot0 && p.slots <= p.frames,
               "rmem_stroke_draw_labels: the pass's slots must be a range of the stroked frames', no longer than its frames");
  RMEM_REQUIRE(p.item0 >= 0 && p.items >= 0 && p.items <= kMaxItems - p.item0, "rmem_stroke_draw_labels: the pass's items must lie in 0..2^31-1");
  RMEM_REQUIRE(p.items == 0 || (p.segs >= 1 && p.strokes >= 1), "rmem_stroke_draw_labels: items need segments and strokes in the pass");
  RMEM_REQUIRE(p.strokes == 0 || p.slots >= 1, "rmem_stroke_draw_labels: strokes need a slot in the pass");
  RMEM_REQUIRE(((uintptr_t)workspace & 15u) == 0, "rmem_stroke_draw_labels: the workspace must be 16-byte aligned");
  RMEM_REQUIRE(((uintptr_t)seg_xy & 15u) == 0, "rmem_stroke_draw_labels: seg_xy must be 16-byte aligned");
  const size_t need = rmem_stroke_workspace_bytes(p.slots, H, W);
  RMEM_REQUIRE(need != 0 && workspace_bytes >= need, "rmem_stroke_draw_labels: the workspace is smaller than rmem_stroke_workspace_bytes says");
  hipStream_t st = (hipStream_t)stream;
  int* owner = (int*)workspace;
  if (p.slots > 0 && hipMemsetAsync(owner, 0, (size_t)p.slots * H * W * 4, st) != hipSuccess) {
    rmem_set_error("rmem_stroke_draw_labels: hipMemsetAsync failed");
    return -1;
  }
  if (p.strokes > 0)
    hipLaunchKernelGGL(k_stroke_check, dim3((unsigned)((p.strokes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, strokes, frame_stroke, stroked,
                       nstrokes, H, W, p, status);
  if (p.segs > 0 && p.strokes > 0)
    hipLaunchKernelGGL(k_stroke_segments, dim3((unsigned)((p.segs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const int4*)seg_xy, seg_stroke,
                       seg_first, strokes, H, W, p, status);
  if (p.items > 0)
    hipLaunchKernelGGL(k_stroke_cover, dim3((unsigned)((p.items + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const int4*)seg_xy, seg_stroke,
                       seg_first, strokes, frame_stroke, (const int*)status, H, W, p, owner);
  const int pieces = (W + 15) / 16 + 1;                               // H * pieces <= H * W / 16 + 2 H
  const long long threads = (long long)H * pieces;
  hipLaunchKernelGGL(k_stroke_paint, dim3((unsigned)((threads + kThreads - 1) / kThreads), (unsigned)p.frames), dim3(kThreads), 0, st, strokes,
                     frame_stroke, stroked, (const int*)status, H, W, pieces, p, (const int*)owner, over, labels);
  return rmem_check_launch("rmem_stroke_draw_labels");
}
