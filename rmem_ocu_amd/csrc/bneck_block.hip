// A whole ResNet bottleneck with planes = 64 (layer 1, stride 1) in ONE launch (gfx950, wave64), NHWC:
//
//   a = relu(conv1x1(x; W1, b1))                       x has Cin = 64 (block 1.0) or 256 (blocks 1.1, 1.2)       (encoders/resnet.py:48-50)
//   b = relu(conv3x3(a; W2, b2)), pad 1                                                                          (encoders/resnet.py:52-56)
//   identity form   (Cin = 256): y = relu(b . W3^T + b3 + x)                                                     (encoders/resnet.py:62-68)
//   projection form (Cin = 64):  y = relu([b | x] . W3cat^T + b3cat)     the packed c3ds weights [256][64 + 64], k order b then x
//   optional tail   (identity):  a_next = relu(y . W1'^T + b1'), N2 = 128: the next layer's first conv1, y rounded exactly as stored
//
// Why: as separate launches (1x1 GEMM, conv3x3_direct.hip, bottleneck.hip) the 64-channel maps a and b make a round trip through HBM
// each (52.8 MB per map at 16 images of 121 x 213) and the chain kernel re-streams 64 KB of weights per 64 pixels.  Here the block's
// input is read once and its output written once; a and b never leave the CU.
//
// Shape: a strip kernel (strip_conv.h).  A workgroup owns a column strip (64 pixels computed, 62 delivered) and walks down a
// run of rows.  A step takes input row r = y + 1:
//   A  the row piece of x (64 pixels, columns x0 - 1 .. x0 + 62, zero fill outside the image) has arrived by LDS-DMA as k-step panels
//      [64 pixels][64 k]; conv1 (W1 in REGISTERS, the A operand) turns it into row r of a in a ring of four row slots in the layout
//      of ring_slot_off.  Where the pixel lies outside the image a is ZERO (the 3x3 pads a, not x: conv1 of a zero pixel would
//      be relu(b1));
//   B  the 3x3 of output row y reads ring rows y - 1 .. y + 1 with W2 in registers (the loop of ring3x3_mfma, written out here: see
//      step B) and leaves b as a [64 pixels][64 k] panel;
//   C  conv3 against W3 resident in LDS (loaded once per workgroup), W3 as the A operand: a lane's accumulators are 4 consecutive
//      channels of a pixel, and the epilogue (+ bias, + shortcut, ReLU, one rounding) runs in registers, without staging or barriers.
//      The identity shortcut is the x row again, fetched by LDS-DMA into the y tile one step after conv1 read it (measured: most of
//      it misses the L2 by then); the projection form keeps its x rows (8 KB each) in a ring of four and reads row y as the second k-step;
//   D  tail: the y tile, rounded as stored, is the B operand of W1' (in registers); it lives in the x buffer that conv1 has just consumed.
// x rows are double-buffered: row r + 2 is requested at the end of step r and waited for (s_waitcnt vmcnt(0)) a whole step later, before
// the stores of step r + 1's epilogue, which then drain behind the following step.  Three barriers a step (four with the tail).
// The halo columns and the two halo rows of every run are recomputed through conv1; outputs do not depend on the partition.
//
// Results are BIT-IDENTICAL to the separate launches: the same 16x16x32 MFMA chains in the same k order, the same epilogue arithmetic,
// a and b rounded to the 16-bit type where the separate launches store them (tests/test_hip_bneck_block.py).
//
// 256 threads = 4 waves, one workgroup per CU (LDS 136 KB, projection form 160 KB); registers: W2 144, W1 8 / 32, W1' 64.
#include "common.h"
#include "lds_dma.h"
#include "strip_conv.h"
#include "../../include/rmem.h"
#include <stdlib.h>

namespace {

constexpr int TP = 64;                          // pixels a step computes ...
constexpr int TPV = 62;                         // ... of which it delivers 62
constexpr int SLOT = TP * 64 * 2;               // a ring row, an x k-step panel, the b panel: 64 pixels x 64 channels
constexpr int BP_B = SLOT;
constexpr int N3 = 256, N2T = 128;

struct BbParams {
  const e16* x; const e16* w1; const float* b1; const e16* w2; const float* b2; const e16* w3; const float* b3; e16* y;
  const e16* w1n; const float* b1n; e16* an;
  int images, H, W, tiles_x, nruns, run_len;
  long x_bytes;
};

template <bool PROJ, bool TAIL>
__global__ __launch_bounds__(256) void k_bneck_block(BbParams p) {
  static_assert(!(PROJ && TAIL), "the tail is built for the identity form");
  constexpr int CIN = PROJ ? 64 : 256, PIXB = CIN * 2;
  constexpr int KS1 = CIN / 32;                 // k-slices of conv1
  constexpr int KT3 = PROJ ? 128 : 64, NK3 = KT3 / 64;
  constexpr int W3_B = N3 * KT3 * 2;
  constexpr int XP_B = PROJ ? 4 * SLOT : 8 * SLOT;     // projection: a ring of four x rows; identity: two x rows of four k-step panels
  constexpr int NSLOT = PROJ ? 3 : 4;           // rows of a: three in use; the identity form has room for a fourth
  constexpr int RING_B = NSLOT * SLOT;
  constexpr int YT_B = PROJ ? 4 * SLOT : 0;     // the y tile [4 k-step panels][64 pixels][64 channels]: identity: the x row that conv1 has consumed
  constexpr int SROW2 = N2T * 2 + 16;           // 16-bit staging row of the tail
  constexpr int NDMA = PROJ ? 2 : 8;            // LDS-DMA requests per thread and x row
  // ONE shared object; the ring comes first: columns 64, 65 of a slot (outputs 62, 63, never stored) read the bytes behind it
  __shared__ __attribute__((aligned(16))) char smem[RING_B + XP_B + BP_B + W3_B + YT_B];
  static_assert(sizeof(smem) <= 160 * 1024, "LDS of a CU");
  char* const ring = smem;
  char* const XP = smem + RING_B;
  char* const BP = XP + XP_B;
  char* const W3s = BP + BP_B;
  auto xbuf = [&](int row) { return XP + (PROJ ? ((row + 1) & 3) * SLOT : (row & 1) * (4 * SLOT)); };
  auto aslot = [&](int row) { return ring + (unsigned)(row + 1) % (unsigned)NSLOT * SLOT; };      // row >= -1

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fc = lane >> 4;
  const int wc = wave >> 1, wp = wave & 1;      // 3x3: channel half, pixel half
  const int wm = wave >> 1, wn = wave & 1;      // conv3: pixel half, channel half
  const int u = blockIdx.x;
  const int xt = u % p.tiles_x, run = (u / p.tiles_x) % p.nruns, img = u / (p.tiles_x * p.nruns);
  const int x0 = xt * TPV, y0 = run * p.run_len, y1 = min(p.H, y0 + p.run_len);
  if (y0 >= y1) return;
  const int npix = min(TPV, p.W - x0);
  // descriptor base = one pixel before image 0, so that column x0 - 1 has a non-negative offset
  const rsrc_t rs = make_rsrc(reinterpret_cast<const char*>(p.x) - PIXB, p.x_bytes + PIXB);
  const rsrc_t rs_w3 = make_rsrc(p.w3, (long)W3_B);

  // ---- per-lane source offsets of the DMA pieces (piece = 8 rows x 128 B; lane = (row, physical chunk)) ----
  int x_off[2], w3_off[8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = 16 * wave + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    x_off[i] = (unsigned)(x0 + r - 1) < (unsigned)p.W ? r * PIXB + c * 16 : OOB;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = 64 * wave + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    w3_off[i] = (r * KT3 + c * 8) * 2;
  }
  // the identity shortcut of output row y: x row y again, shifted by one pixel (tile pixel px is column x0 + px) into the
  // buffer that becomes the y tile; every wave requests exactly the region its own epilogue reads: pixels wm * 32 .., channels wn * 128 ..
  int sc_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 32 * wm + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    sc_off[i] = x0 + r < p.W ? (r + 1) * PIXB + c * 16 : OOB;
  }
  auto issue_sc = [&](int row, char* dst) {
    const int base = ((img * p.H + row) * p.W + x0) * PIXB;
#pragma unroll
    for (int kp = 0; kp < 2; ++kp)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        buf_load_lds16(rs, (lptr_t)(dst + (2 * wn + kp) * SLOT + (32 * wm + 8 * i) * 128), sc_off[i], base + (2 * wn + kp) * 128);
  };
  auto issue_x = [&](int row) {                 // input row `row` of the strip (rows outside the image or past the run's halo: zero fill)
    const bool ok = (unsigned)row < (unsigned)p.H && row <= y1;
    const int base = ((img * p.H + (ok ? row : 0)) * p.W + x0) * PIXB;
    char* dst = xbuf(row);
#pragma unroll
    for (int kp = 0; kp < CIN / 64; ++kp)
#pragma unroll
      for (int i = 0; i < 2; ++i) buf_load_lds16(rs, (lptr_t)(dst + kp * SLOT + (16 * wave + 8 * i) * 128), ok ? x_off[i] : OOB, base + kp * 128);
  };

#pragma unroll
  for (int kt = 0; kt < NK3; ++kt)
#pragma unroll
    for (int i = 0; i < 8; ++i) buf_load_lds16(rs_w3, (lptr_t)(W3s + kt * (N3 * 128) + (64 * wave + 8 * i) * 128), w3_off[i], kt * 128);
  issue_x(y0 - 1);
  issue_x(y0);
  __builtin_amdgcn_sched_barrier(0);

  // ---- weights that live in registers ----
  // W1 [64][CIN], the A operand of conv1: this wave's 16 output channels, lane -> channel 16 wave + (lane & 15), k = 32 slice + 8 (lane >> 4) ..
  e16x8 w1f[KS1];
#pragma unroll
  for (int ks = 0; ks < KS1; ++ks) w1f[ks] = *reinterpret_cast<const e16x8*>(p.w1 + (16 * wave + fr) * CIN + ks * 32 + fc * 8);
  const f32x4 bv1 = *reinterpret_cast<const f32x4*>(p.b1 + 16 * wave + fc * 4);
  // W2 [64][3][3][64], the A operand of the 3x3: 2 x 18 fragments of this wave's 32 output channels
  e16x8 wf[2][18];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) wf[ct][ks] = *reinterpret_cast<const e16x8*>(p.w2 + ((wc * 2 + ct) * 16 + fr) * 576 + ks * 32 + fc * 8);
  f32x4 bv2[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) bv2[ct] = *reinterpret_cast<const f32x4*>(p.b2 + (wc * 2 + ct) * 16 + fc * 4);
  // W1' [128][256], the A operand of the tail: this wave's 32 output channels
  e16x8 wnf[TAIL ? 2 : 1][TAIL ? 8 : 1];
  f32x4 bvn[2];
  if constexpr (TAIL) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) wnf[ct][ks] = *reinterpret_cast<const e16x8*>(p.w1n + (32 * wave + 16 * ct + fr) * N3 + ks * 32 + fc * 8);
      bvn[ct] = *reinterpret_cast<const f32x4*>(p.b1n + 32 * wave + 16 * ct + fc * 4);
    }
  }
  // conv3: this wave's 32 pixels (2 tiles) x 128 channels (8 tiles); a lane finishes channels wn * 128 + 16 j + 4 fc .. + 3 of pixel wm * 32 + 16 i + fr
  f32x4 bias3[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bias3[j] = *reinterpret_cast<const f32x4*>(p.b3 + wn * 128 + j * 16 + fc * 4);

  // byte offset of this lane's (pixel, chunk fc) inside a ring slot under horizontal tap dx, channel slice 0
  int coff[2][3];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) coff[pt][dx] = ring_slot_off<8>((wp * 2 + pt) * 16 + fr + dx, fc);
  // where conv1 puts its 4 channels (16 wave + 4 fc ..: chunk 2 wave + (fc >> 1), a chunk being 256 bytes on from the one before, and
  // the half fc & 1 of it) of pixel 16 pt + fr in a ring slot, and whether that pixel is inside the image
  int aoff[4];
  bool acol[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int col = pt * 16 + fr;
    aoff[pt] = ring_slot_off<8>(col, 2 * wave) + (fc >> 1) * 256 + (fc & 1) * 8;
    acol[pt] = (unsigned)(x0 + col - 1) < (unsigned)p.W;
  }
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int r = y0 - 1; r <= y1; ++r) {
    // ---- A: row r of a = relu(x row . W1^T + b1), zero outside the image ----
    {
      const char* xp = xbuf(r);
      f32x4 acc1[4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc1[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      e16x8 bf[2][4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) bf[0][pt] = *reinterpret_cast<const e16x8*>(xp + swz(pt * 16 + fr, fc) * 2);
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks) {
        if (ks + 1 < KS1) {
          const e16* panel = reinterpret_cast<const e16*>(xp + ((ks + 1) >> 1) * SLOT);
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) bf[(ks + 1) & 1][pt] = *reinterpret_cast<const e16x8*>(&panel[swz(pt * 16 + fr, 4 * ((ks + 1) & 1) + fc)]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc1[pt] = RMEM_MFMA_16x16x32(w1f[ks], bf[ks & 1][pt], acc1[pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      const bool rowok = (unsigned)r < (unsigned)p.H;
      char* slot = aslot(r);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const bool ok = rowok && acol[pt];
        e16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ok ? (e16)fmaxf(acc1[pt][j] + bv1[j], 0.f) : (e16)0.f;
        *reinterpret_cast<e16x4*>(slot + aoff[pt]) = o;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();               // row r of a is complete; every wave has read the x row
    if (r <= y0) {                              // the two rows above the first output row: no output yet
      issue_x(r + 2);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");      // row r + 1 has landed (everything but the requests just made)
      __builtin_amdgcn_s_barrier();
      continue;
    }
    const int y = r - 1;
    const long pix0 = ((long)img * p.H + y) * p.W + x0;

    char* const YTb = PROJ ? W3s + W3_B : xbuf(r);      // identity: the x row that conv1 has consumed
    e16* const Yt = reinterpret_cast<e16*>(YTb);
    if constexpr (!PROJ) issue_sc(y, YTb);

    // ---- B: b = relu(conv3x3(a) + b2) of output row y: the loop of ring3x3_mfma<2, 2, 2> (strip_conv.h) ----
    // (written out: called as that function the identity forms of this kernel compile to 4 more registers and another order of
    // waits, profiles/strip_conv_isa.txt; a kernel that calls ring3x3_mfma from the start has no such parity to keep)
    {
      f32x4 acc[2][2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char* rb[3];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) rb[dy] = aslot(y - 1 + dy);
      e16x8 bf[2][2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) bf[0][pt] = *reinterpret_cast<const e16x8*>(rb[0] + coff[pt][0]);
#pragma unroll
      for (int k = 0; k < 18; ++k) {
        if (k + 1 < 18) {
          const int tap = (k + 1) / 2, s = (k + 1) % 2, dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) bf[(k + 1) & 1][pt] = *reinterpret_cast<const e16x8*>(rb[dy] + coff[pt][dx] + s * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) acc[ct][pt] = RMEM_MFMA_16x16x32(wf[ct][k], bf[k & 1][pt], acc[ct][pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      e16* Bp = reinterpret_cast<e16*>(BP);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          e16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (e16)fmaxf(acc[ct][pt][j] + bv2[ct][j], 0.f);
          const int px = (wp * 2 + pt) * 16 + fr;
          *reinterpret_cast<e16x4*>(&Bp[swz(px, (wc * 2 + ct) * 2 + (fc >> 1)) + (fc & 1) * 4]) = o;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // ---- C: y = relu([b | x] . W3^T + b3 (+ x)), W3 the A operand ----
    f32x4 acc3[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc3[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NK3; ++kt) {
      // the projection's second k-step: row y of x; output pixel px is column px + 1 of the x row piece
      const e16* Ps = reinterpret_cast<const e16*>(kt == 0 ? BP : xbuf(y));
      const int sh = kt == 0 ? 0 : 1;
      const e16* Ws = reinterpret_cast<const e16*>(W3s + kt * (N3 * 128));
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        e16x8 pf[2], wfr[8];
#pragma unroll
        for (int i = 0; i < 2; ++i) pf[i] = *reinterpret_cast<const e16x8*>(&Ps[swz(wm * 32 + i * 16 + fr + sh, 4 * ks + fc)]);
#pragma unroll
        for (int j = 0; j < 8; ++j) wfr[j] = *reinterpret_cast<const e16x8*>(&Ws[swz(wn * 128 + j * 16 + fr, 4 * ks + fc)]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc3[i][j] = RMEM_MFMA_16x16x32(wfr[j], pf[i], acc3[i][j], 0, 0, 0);
      }
    }
    // x row r + 1 (requested a step ago) and this wave's part of the shortcut have landed; the barriers below make every wave's
    // pieces of the x row visible
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the epilogue, in place: a lane replaces the 4 shortcut channels of its pixel by y, rounded as stored
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int px = wm * 32 + i * 16 + fr;
      e16x4 sc[8];
      if constexpr (!PROJ) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int n = wn * 128 + j * 16 + fc * 4;
          sc[j] = *reinterpret_cast<const e16x4*>(&Yt[(n >> 6) * (TP * 64) + swz(px, (n >> 3) & 7) + (n & 7)]);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = wn * 128 + j * 16 + fc * 4;
        e16x4 o;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          float v = acc3[i][j][rr] + bias3[j][rr];
          if constexpr (!PROJ) v += (float)sc[j][rr];
          o[rr] = (e16)fmaxf(v, 0.f);
        }
        *reinterpret_cast<e16x4*>(&Yt[(n >> 6) * (TP * 64) + swz(px, (n >> 3) & 7) + (n & 7)]) = o;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();               // the y tile is complete
    // y in rows: 32 lanes store the 512 contiguous bytes of a pixel
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = tid + 256 * j, px = q >> 5, c = q & 31;
      const e16x8 o = *reinterpret_cast<const e16x8*>(&Yt[(c >> 3) * (TP * 64) + swz(px, c & 7)]);
      if (px < npix) *reinterpret_cast<e16x8*>(p.y + (pix0 + px) * N3 + c * 8) = o;
    }

    // ---- D: a_next = relu(y tile . W1'^T + b1'), W1' in registers ----
    if constexpr (TAIL) {
      f32x4 acc2[2][4];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc2[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      e16x8 bf[2][4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) bf[0][pt] = *reinterpret_cast<const e16x8*>(&Yt[swz(pt * 16 + fr, fc)]);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks + 1 < 8) {
          const e16* panel = Yt + ((ks + 1) >> 1) * (TP * 64);
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) bf[(ks + 1) & 1][pt] = *reinterpret_cast<const e16x8*>(&panel[swz(pt * 16 + fr, 4 * ((ks + 1) & 1) + fc)]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) acc2[ct][pt] = RMEM_MFMA_16x16x32(wnf[ct][ks], bf[ks & 1][pt], acc2[ct][pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();             // every wave has read the y tile: it becomes the 16-bit staging rows of a_next
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
          e16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (e16)fmaxf(acc2[ct][pt][j] + bvn[ct][j], 0.f);
          *reinterpret_cast<e16x4*>(YTb + (pt * 16 + fr) * SROW2 + (32 * wave + 16 * ct + fc * 4) * 2) = o;
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = tid + 256 * j, px = v >> 4, c16 = v & 15;
        const e16x8 o = *reinterpret_cast<const e16x8*>(YTb + px * SROW2 + c16 * 16);
        if (px < npix) *reinterpret_cast<e16x8*>(p.an + (pix0 + px) * N2T + c16 * 8) = o;
      }
    }
    // every wave has waited for its pieces of x row r + 1 and is done with the b panel, the y tile (its buffer takes x row r + 2) and
    // (projection) x row r - 1
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue_x(r + 2);
  }
}

}  // namespace

extern "C" int RMEM_API(rmem_bneck_block64)(const rmem_bneck_block_desc* d, const void* x, const void* w1, const float* bias1, const void* w2,
                                            const float* bias2, const void* w3, const float* bias3, void* y, const void* w1n, const float* bias1n,
                                            void* a_next, void* stream) {
  RMEM_REQUIRE(d && x && w1 && bias1 && w2 && bias2 && w3 && bias3 && y, "rmem_bneck_block64: null argument");
  RMEM_REQUIRE(d->images >= 1 && d->H >= 1 && d->W >= 1 && (d->Cin == 64 || d->Cin == 256),
               "rmem_bneck_block64: Cin must be 64 (projection form) or 256 (identity form)");
  RMEM_REQUIRE(d->N2 == 0 || (d->N2 == 128 && d->Cin == 256), "rmem_bneck_block64: the tail needs N2 = 128 and the identity form");
  RMEM_REQUIRE((d->N2 != 0) == (w1n != nullptr) && (d->N2 != 0) == (bias1n != nullptr) && (d->N2 != 0) == (a_next != nullptr),
               "rmem_bneck_block64: w1n, bias1n and a_next go with N2 != 0");
  RMEM_REQUIRE(rmem_al16(x) && rmem_al16(w1) && rmem_al16(bias1) && rmem_al16(w2) && rmem_al16(bias2) && rmem_al16(w3) && rmem_al16(bias3) &&
               rmem_al16(y) && rmem_al16(w1n) && rmem_al16(bias1n) && rmem_al16(a_next), "rmem_bneck_block64: operands must be 16-byte aligned");
  BbParams p;
  p.x = (const e16*)x; p.w1 = (const e16*)w1; p.b1 = bias1; p.w2 = (const e16*)w2; p.b2 = bias2; p.w3 = (const e16*)w3; p.b3 = bias3;
  p.y = (e16*)y; p.w1n = (const e16*)w1n; p.b1n = bias1n; p.an = (e16*)a_next;
  p.images = d->images; p.H = d->H; p.W = d->W;
  p.tiles_x = (d->W + TPV - 1) / TPV;
  p.x_bytes = (long)d->images * d->H * d->W * d->Cin * 2;
  RMEM_REQUIRE(p.x_bytes + (long)(d->W + TP + 2) * d->Cin * 2 < kRsrcLimit, "rmem_bneck_block64: the input exceeds the 2 GB a buffer descriptor addresses");
  // runs of output rows per column strip: one workgroup per CU, rows per run as long as that allows (every run recomputes 2 rows of a
  // and re-loads the weights); RMEM_BNECK_ROWS forces the rows per run (tests: 1, 2, or >= H for the whole image)
  const int wgs = rmem_env_int("RMEM_BNECK_WGS", 256);
  const int forced = rmem_env_int("RMEM_BNECK_ROWS", 0);
  const long strips = (long)d->images * p.tiles_x;
  const StripRuns runs = strip_runs(wgs, strips, d->H, forced);
  p.nruns = runs.nruns; p.run_len = runs.run_len;
  const long grid = strips * p.nruns;
  RMEM_REQUIRE(grid < (1L << 30), "rmem_bneck_block64: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  if (d->Cin == 64) hipLaunchKernelGGL((k_bneck_block<true, false>), dim3((unsigned)grid), dim3(256), 0, s, p);
  else if (d->N2) hipLaunchKernelGGL((k_bneck_block<false, true>), dim3((unsigned)grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((k_bneck_block<false, false>), dim3((unsigned)grid), dim3(256), 0, s, p);
  return rmem_check_launch("rmem_bneck_block64");
}
