// Baseline-JPEG files written on the device (include/rmem.h, rmem_jpeg_encode_* and rmem_overlay_rgb8): uint8 RGB frames, and
// optionally uint8 label maps that are overlaid first, in; complete .jpg files packed back to back out.
//
// The files are libjpeg-turbo's bit for bit at 4:2:0 with the standard tables (the rules are in include/rmem.h).  Nothing in the
// format needs a table built from the data, so the encoder is transform, count bits, scan, emit, stuff:
//   k_jenc_mcu     one workgroup per 4 MCUs, one thread per 2x2 pixel quad: overlay (labels read with their 4-neighbours), colour
//                  conversion, the h2v2 average -- edge replication is a clamp of the coordinates -- into LDS; then 8 lanes per
//                  block run the ISLOW FDCT (row pass, LDS, column pass), quantise, and the workgroup writes its 24 blocks as
//                  int16 in zig-zag order, dummy blocks filled in.  Blocks are stored in scan order: block = 6 * MCU + k.
//   k_jenc_size    one thread per block: the DC difference (predecessor in scan order, reset at an interval's first MCU) and the
//                  block's bit count.
//   k_jenc_scan    one workgroup per restart interval: exclusive scan of its blocks' bits (in place), the interval's bit total,
//                  and zeroes of the words of the interval's slice of the raw buffer that the bits will touch.
//   k_jenc_emit    one thread per block: its codes at its bit offset, most significant bit first.  Ownership rule as in png.hip:
//                  a 32-bit word wholly inside one block's bits is a plain store, a word shared with a neighbouring block is
//                  OR-ed into the zeroed memory with a vector atomic.  The interval's last block adds the 1-bits of the padding.
//   k_jenc_count   one workgroup per interval: the 0xFF bytes of its raw bytes -> its size in the file (+ 2 for a marker).
//   k_jenc_frames  one workgroup per frame: exclusive scan of the interval sizes; the frame's file size.
//   k_codec_offsets (codec.h) one workgroup: exclusive scan of the file sizes -> offsets[0..frames].
//   k_jenc_place   one workgroup per interval: its raw bytes to their final place, 0x00 after every 0xFF, then RSTm; the first
//                  interval's workgroup also copies the header, the last one's writes EOI.
// The restart interval and the header travel in the device table blob (rmem_jpeg_encode_header); the host sizes every grid
// for the most intervals a frame can have (one per MCU row) and workgroups beyond the blob's count leave at once.
// All arithmetic is 32-bit integer; the largest FDCT intermediate is below 2^30 for 8-bit input.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include "common.h"
#include "codec.h"
#include "../../include/rmem.h"

namespace {

constexpr int kBlockBits = 22 + 63 * 26;          // DC: 11-bit code + 11 bits; AC: 16-bit code + 10 bits
constexpr int kBlockBytes = (kBlockBits + 7) / 8;  // 208
// table blob, 32-bit words
constexpr int kTabQ = 0;        // 2 x 64 divisors 8 Q, natural order (luma, chroma)
constexpr int kTabDc = 128;     // 2 x 16 (length << 16 | code) per size category
constexpr int kTabAc = 160;     // 2 x 256 per run/size symbol
constexpr int kTabRestart = 672, kTabHeaderLen = 673, kTabH = 674, kTabW = 675, kTabHeader = 676;
constexpr int kTabWords = RMEM_JPEG_ENC_TABLE_BYTES / 4;
constexpr int kMcusPerGroup = 4;

const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__constant__ unsigned char c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const unsigned char kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                                  69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                                  81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                    99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: number of codes of each length 1..16, then the symbols in code order
const unsigned char kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const unsigned char kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const unsigned char kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const unsigned char kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct Geo {
  int H, W, mcus_x, mcus_y, mcus, wib_y, hib_y, ch;   // wib_y / hib_y: real luma blocks; ch: real chroma rows
  long nblk;                                          // blocks of one frame: 6 per MCU
  long row_words;                                     // raw-buffer words of one MCU row (worst case + 2)
};

__host__ __device__ inline Geo make_geo(int H, int W) {
  Geo g;
  g.H = H;
  g.W = W;
  g.mcus_x = (W + 15) / 16;
  g.mcus_y = (H + 15) / 16;
  g.mcus = g.mcus_x * g.mcus_y;
  g.wib_y = (W + 7) / 8;
  g.hib_y = (H + 7) / 8;
  g.ch = (H + 1) / 2;
  g.nblk = 6L * g.mcus;
  g.row_words = ((long)g.mcus_x * 6 * kBlockBits + 31) / 32 + 2;
  return g;
}

// MCU rows per restart interval and the number of intervals, from the blob's restart_rows (0 = none)
__device__ __forceinline__ void intervals_of(const Geo& g, int restart_rows, int& rows_per, int& nint) {
  rows_per = (restart_rows <= 0 || restart_rows > g.mcus_y) ? g.mcus_y : restart_rows;
  nint = (g.mcus_y + rows_per - 1) / rows_per;
}

// ---------------------------------------------------------------------------------------------------------------- overlay
// the pixel (y, x) of the overlaid frame: black where a 4-neighbour inside the image carries a larger label, else the palette blend
// for a label != 0, else the pixel itself
__device__ __forceinline__ void overlay_pixel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ lab, const uint8_t* pal,
                                              int a, int H, int W, int y, int x, int& r, int& g, int& b) {
  const long p = (long)y * W + x;
  r = rgb[3 * p];
  g = rgb[3 * p + 1];
  b = rgb[3 * p + 2];
  if (!lab) return;
  const int l = lab[p];
  int m = 0;
  if (y > 0) m = max(m, (int)lab[p - W]);
  if (y + 1 < H) m = max(m, (int)lab[p + W]);
  if (x > 0) m = max(m, (int)lab[p - 1]);
  if (x + 1 < W) m = max(m, (int)lab[p + 1]);
  if (m > l) {
    r = g = b = 0;
  } else if (l) {
    const int ia = 256 - a;
    r = (a * r + ia * pal[3 * l] + 128) >> 8;
    g = (a * g + ia * pal[3 * l + 1] + 128) >> 8;
    b = (a * b + ia * pal[3 * l + 2] + 128) >> 8;
  }
}

__global__ __launch_bounds__(256) void k_overlay(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ labels,
                                                 const uint8_t* __restrict__ palette, int a, int H, int W, uint8_t* __restrict__ out) {
  __shared__ uint8_t s_pal[768];
  for (int i = threadIdx.x; i < 768; i += 256) s_pal[i] = palette[i];
  __syncthreads();
  const long hw = (long)H * W, f = blockIdx.y;
  const uint8_t* frgb = rgb + f * hw * 3;
  const uint8_t* flab = labels + f * hw;
  uint8_t* fout = out + f * hw * 3;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    int r, g, b;
    overlay_pixel(frgb, flab, s_pal, a, H, W, y, x, r, g, b);
    fout[3 * p] = (uint8_t)r;
    fout[3 * p + 1] = (uint8_t)g;
    fout[3 * p + 2] = (uint8_t)b;
  }
}

// ---------------------------------------------------------------------------------------------------------------- MCU stage
// one jfdctint.c pass over d[0..7]; FIRST: the row pass (results scaled up by PASS1_BITS = 2)
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
  constexpr int n = FIRST ? 11 : 15, rnd = 1 << (n - 1);
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) << 2;
    d[4] = (t10 - t11) << 2;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = (z1 + t13 * 6270 + rnd) >> n;
  d[6] = (z1 - t12 * 15137 + rnd) >> n;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = (a4 + z1 + z3 + rnd) >> n;
  d[5] = (a5 + z2 + z4 + rnd) >> n;
  d[3] = (a6 + z2 + z3 + rnd) >> n;
  d[1] = (a7 + z1 + z4 + rnd) >> n;
}

constexpr int kBlkStride = 72;      // 8 rows of 9 words: the row and the column pass both spread over the LDS banks

__global__ __launch_bounds__(256) void k_jenc_mcu(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ labels,
                                                  const uint8_t* __restrict__ palette, int a, Geo g, const uint32_t* __restrict__ tab,
                                                  int16_t* __restrict__ coef) {
  __shared__ int s_blk[kMcusPerGroup * 6 * kBlkStride];
  __shared__ uint8_t s_pal[768];
  __shared__ uint16_t s_q[128];
  const int tid = threadIdx.x;
  if (labels)
    for (int i = tid; i < 768; i += 256) s_pal[i] = palette[i];
  if (tid < 128) s_q[tid] = (uint16_t)tab[kTabQ + tid];
  __syncthreads();
  const long f = blockIdx.y, hw = (long)g.H * g.W;
  const uint8_t* frgb = rgb + f * hw * 3;
  const uint8_t* flab = labels ? labels + f * hw : nullptr;
  const int mcu0 = blockIdx.x * kMcusPerGroup;
  {  // one 2x2 quad per thread: four luma samples, one Cb, one Cr
    const int lm = tid >> 6, q = tid & 63, qy = q >> 3, qx = q & 7;
    const int mcu = min(mcu0 + lm, g.mcus - 1);
    const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
    const int cy = min(my * 8 + qy, g.ch - 1);                  // chroma rows below the last real one repeat it
    int sb = 0, sr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int px = min(mx * 16 + 2 * qx + dx, g.W - 1);
        const int ly = min(my * 16 + 2 * qy + dy, g.H - 1), cyy = min(2 * cy + dy, g.H - 1);
        int r, gg, b;
        overlay_pixel(frgb, flab, s_pal, a, g.H, g.W, ly, px, r, gg, b);
        const int Y = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
        const int yy = 2 * qy + dy, xx = 2 * qx + dx;
        s_blk[(lm * 6 + (yy >> 3) * 2 + (xx >> 3)) * kBlkStride + (yy & 7) * 9 + (xx & 7)] = Y - 128;
        if (cyy != ly) overlay_pixel(frgb, flab, s_pal, a, g.H, g.W, cyy, px, r, gg, b);
        sb += (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
        sr += (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
      }
    const int bias = 1 + (qx & 1);
    s_blk[(lm * 6 + 4) * kBlkStride + qy * 9 + qx] = ((sb + bias) >> 2) - 128;
    s_blk[(lm * 6 + 5) * kBlkStride + qy * 9 + qx] = ((sr + bias) >> 2) - 128;
  }
  __syncthreads();
  const int blk = tid >> 3, l8 = tid & 7;                        // 24 blocks x 8 lanes
  int d[8];
  if (blk < kMcusPerGroup * 6) {
    int* p = s_blk + blk * kBlkStride + l8 * 9;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i];
    fdct_1d<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = d[i];
  }
  __syncthreads();
  if (blk < kMcusPerGroup * 6) {
    int* p = s_blk + blk * kBlkStride + l8;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i * 9];
    fdct_1d<false>(d);
    const uint16_t* q = s_q + ((blk % 6) >= 4 ? 64 : 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int dv = q[i * 8 + l8], c = d[i], m = (abs(c) + (dv >> 1)) / dv;
      p[i * 9] = c < 0 ? -m : m;
    }
  }
  __syncthreads();
  // the strip's blocks, int16, zig-zag order, two coefficients per 32-bit store
  const int nm = min(kMcusPerGroup, g.mcus - mcu0);
  uint32_t* dst = (uint32_t*)(coef + (f * g.nblk + (long)mcu0 * 6) * 64);
  for (int w = tid; w < nm * 6 * 32; w += 256) {
    const int b = w >> 5, k = (w & 31) * 2, lm = b / 6, kb = b - lm * 6;
    const int mcu = mcu0 + lm, my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
    const bool dumcol = 2 * mx + 1 >= g.wib_y, dumrow = 2 * my + 1 >= g.hib_y;
    // jccoefct.c: a dummy block has no ACs and the DC of the block before it in the MCU
    int src = kb;
    if (kb == 1) src = dumcol ? 0 : 1;
    else if (kb == 2) src = dumrow ? (dumcol ? 0 : 1) : 2;
    else if (kb == 3) src = dumrow ? (dumcol ? 0 : 1) : (dumcol ? 2 : 3);
    const bool dummy = kb < 4 && (((kb & 1) && dumcol) || ((kb & 2) && dumrow));
    const int* sp = s_blk + (lm * 6 + src) * kBlkStride;
    int v0, v1;
    if (dummy) {
      v0 = k == 0 ? sp[0] : 0;
      v1 = 0;
    } else {
      const int n0 = c_zigzag[k], n1 = c_zigzag[k + 1];
      v0 = sp[(n0 >> 3) * 9 + (n0 & 7)];
      v1 = sp[(n1 >> 3) * 9 + (n1 & 7)];
    }
    dst[w] = (uint32_t)(v0 & 0xFFFF) | ((uint32_t)v1 << 16);
  }
}

// ---------------------------------------------------------------------------------------------------------------- entropy coding
__device__ __forceinline__ int size_of(int v) { return 32 - __clz(abs(v)); }   // 0 for 0

// the DC difference of block `b` (scan order) of a frame; pred resets on the interval's first MCU
__device__ __forceinline__ int dc_diff(const int16_t* __restrict__ fcoef, long b, int per_mcus) {
  const long mcu = b / 6;
  const int kb = (int)(b - mcu * 6);
  const int dc = fcoef[b * 64];
  const bool first = mcu % per_mcus == 0;
  if (kb >= 1 && kb <= 3) return dc - fcoef[(b - 1) * 64];
  if (first) return dc;
  return dc - fcoef[(b - (kb == 0 ? 3 : 6)) * 64];
}

__global__ __launch_bounds__(256) void k_jenc_size(const int16_t* __restrict__ coef, Geo g, const uint32_t* __restrict__ tab,
                                                   uint32_t* __restrict__ bbits) {
  __shared__ uint8_t s_len[2][16 + 256];
  for (int i = threadIdx.x; i < 2 * 272; i += 256) {
    const int t = i / 272, s = i - t * 272;
    s_len[t][s] = (uint8_t)((s < 16 ? tab[kTabDc + t * 16 + s] : tab[kTabAc + t * 256 + s - 16]) >> 16);
  }
  __syncthreads();
  int rows_per, nint;
  intervals_of(g, (int)tab[kTabRestart], rows_per, nint);
  const long f = blockIdx.y;
  const int16_t* fcoef = coef + f * g.nblk * 64;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < g.nblk; b += (long)gridDim.x * 256) {
    const int t = (b % 6) >= 4;
    const int s = size_of(dc_diff(fcoef, b, rows_per * g.mcus_x));
    unsigned bits = s_len[t][s] + s;
    const uint4* cw = (const uint4*)(fcoef + b * 64);
    int run = 0;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
      const uint4 v = cw[i];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (i == 0 && j == 0) continue;
        const int c = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
        if (c == 0) {
          ++run;
        } else {
          bits += (run >> 4) * s_len[t][16 + 0xF0];
          const int sz = size_of(c);
          bits += s_len[t][16 + ((run & 15) << 4 | sz)] + sz;
          run = 0;
        }
      }
    }
    if (run) bits += s_len[t][16];
    bbits[f * g.nblk + b] = bits;
  }
}

// one workgroup per (interval, frame)
__global__ __launch_bounds__(256) void k_jenc_scan(uint32_t* __restrict__ bbits, Geo g, const uint32_t* __restrict__ tab,
                                                   uint32_t* __restrict__ ibits, uint32_t* __restrict__ raw) {
  __shared__ unsigned s_wave[4];
  int rows_per, nint;
  intervals_of(g, (int)tab[kTabRestart], rows_per, nint);
  const int it = blockIdx.x;
  if (it >= nint) return;
  const long f = blockIdx.y;
  const int row0 = it * rows_per, rows = min(rows_per, g.mcus_y - row0);
  const long b0 = (long)row0 * g.mcus_x * 6, nb = (long)rows * g.mcus_x * 6;
  uint32_t* fb = bbits + f * g.nblk + b0;
  unsigned carry = 0;
  for (long i0 = 0; i0 < nb; i0 += 256) {
    const long i = i0 + threadIdx.x;
    const unsigned at = block_excl_scan(i < nb ? fb[i] : 0u, s_wave, carry);
    if (i < nb) fb[i] = at;
  }
  if (threadIdx.x == 0) ibits[f * g.mcus_y + it] = carry;
  // the words the interval's bits (and their padding) touch; the slice holds rows * row_words >= this many
  uint32_t* slice = raw + ((size_t)f * g.mcus_y + row0) * g.row_words;
  const long words = ((long)carry + 7 + 31) / 32;
  for (long i = threadIdx.x; i < words; i += 256) slice[i] = 0;
}

// most-significant-bit-first writer of one lane into big-endian 32-bit words: see the ownership rule at the head of this file
struct MsbWriter {
  uint32_t* w;
  uint64_t acc;
  int nb;
  bool shared;
  __device__ __forceinline__ MsbWriter(uint32_t* words, uint32_t bitpos) : w(words + (bitpos >> 5)), acc(0), nb((int)(bitpos & 31)) {
    shared = nb != 0;
  }
  __device__ __forceinline__ void put(uint32_t code, int len) {      // len <= 26
    acc = (acc << len) | code;
    nb += len;
    if (nb >= 32) {
      nb -= 32;
      const uint32_t x = __builtin_bswap32((uint32_t)(acc >> nb));
      if (shared) {
        if (x) atomicOr(w, x);
      } else {
        *w = x;
      }
      shared = false;
      ++w;
      acc &= (1ull << nb) - 1ull;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nb > 0) {
      const uint32_t x = __builtin_bswap32((uint32_t)(acc << (32 - nb)));
      if (x) atomicOr(w, x);
    }
  }
};

__device__ __forceinline__ uint32_t value_bits(int v, int s) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u); }

__global__ __launch_bounds__(256) void k_jenc_emit(const int16_t* __restrict__ coef, Geo g, const uint32_t* __restrict__ tab,
                                                   const uint32_t* __restrict__ bbits, const uint32_t* __restrict__ ibits,
                                                   uint32_t* __restrict__ raw) {
  __shared__ uint32_t s_code[2][16 + 256];
  for (int i = threadIdx.x; i < 2 * 272; i += 256) {
    const int t = i / 272, s = i - t * 272;
    s_code[t][s] = s < 16 ? tab[kTabDc + t * 16 + s] : tab[kTabAc + t * 256 + s - 16];
  }
  __syncthreads();
  int rows_per, nint;
  intervals_of(g, (int)tab[kTabRestart], rows_per, nint);
  const long f = blockIdx.y;
  const int16_t* fcoef = coef + f * g.nblk * 64;
  const long per_blocks = (long)rows_per * g.mcus_x * 6;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < g.nblk; b += (long)gridDim.x * 256) {
    const int t = (b % 6) >= 4;
    const int it = (int)(b / per_blocks);
    uint32_t* slice = raw + ((size_t)f * g.mcus_y + (size_t)it * rows_per) * g.row_words;
    MsbWriter bw(slice, bbits[f * g.nblk + b]);
    const int diff = dc_diff(fcoef, b, rows_per * g.mcus_x);
    int s = size_of(diff);
    uint32_t e = s_code[t][s];
    bw.put((e & 0xFFFF) << s | value_bits(diff, s), (int)(e >> 16) + s);
    const uint4* cw = (const uint4*)(fcoef + b * 64);
    int run = 0;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
      const uint4 v = cw[i];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (i == 0 && j == 0) continue;
        const int c = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
        if (c == 0) {
          ++run;
        } else {
          e = s_code[t][16 + 0xF0];
          for (; run > 15; run -= 16) bw.put(e & 0xFFFF, (int)(e >> 16));
          s = size_of(c);
          e = s_code[t][16 + (run << 4 | s)];
          bw.put((e & 0xFFFF) << s | value_bits(c, s), (int)(e >> 16) + s);
          run = 0;
        }
      }
    }
    if (run) {
      e = s_code[t][16];
      bw.put(e & 0xFFFF, (int)(e >> 16));
    }
    const bool last = b + 1 == g.nblk || (b + 1) % per_blocks == 0;
    if (last) {                                                       // pad the interval to a byte with 1-bits
      const int pad = (8 - (int)(ibits[f * g.mcus_y + it] & 7)) & 7;
      if (pad) bw.put((1u << pad) - 1u, pad);
    }
    bw.finish();
  }
}

__global__ __launch_bounds__(256) void k_jenc_count(Geo g, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ ibits,
                                                    const uint32_t* __restrict__ raw, uint32_t* __restrict__ isize) {
  __shared__ unsigned s_wave[4];
  int rows_per, nint;
  intervals_of(g, (int)tab[kTabRestart], rows_per, nint);
  const int it = blockIdx.x;
  if (it >= nint) return;
  const long f = blockIdx.y;
  const uint32_t* slice = raw + ((size_t)f * g.mcus_y + (size_t)it * rows_per) * g.row_words;
  const long nbytes = ((long)ibits[f * g.mcus_y + it] + 7) / 8;
  unsigned n = 0;
  for (long w = threadIdx.x; w * 4 < nbytes; w += 256) {
    const uint32_t x = slice[w];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (w * 4 + k < nbytes && ((x >> (8 * k)) & 255u) == 255u) ++n;
  }
  n = group_sum(n, s_wave);
  if (threadIdx.x == 0) isize[f * g.mcus_y + it] = (uint32_t)nbytes + n + (it + 1 < nint ? 2u : 0u);
}

// one workgroup per frame: interval sizes -> their byte offsets inside the frame's scan (in place), and the file's size
__global__ __launch_bounds__(256) void k_jenc_frames(Geo g, const uint32_t* __restrict__ tab, uint32_t* __restrict__ isize,
                                                     unsigned long long* __restrict__ fsize) {
  __shared__ unsigned s_wave[4];
  int rows_per, nint;
  intervals_of(g, (int)tab[kTabRestart], rows_per, nint);
  const long f = blockIdx.x;
  uint32_t* fi = isize + f * g.mcus_y;
  unsigned carry = 0;
  for (int i0 = 0; i0 < nint; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const unsigned at = block_excl_scan(i < nint ? fi[i] : 0u, s_wave, carry);
    if (i < nint) fi[i] = at;
  }
  if (threadIdx.x == 0) fsize[f] = (unsigned long long)tab[kTabHeaderLen] + carry + 2;
}

__global__ __launch_bounds__(256) void k_jenc_place(Geo g, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ ibits,
                                                    const uint32_t* __restrict__ ioff, const uint32_t* __restrict__ raw,
                                                    const long long* __restrict__ offsets, uint8_t* __restrict__ out) {
  __shared__ unsigned s_wave[4];
  int rows_per, nint;
  intervals_of(g, (int)tab[kTabRestart], rows_per, nint);
  const int it = blockIdx.x;
  if (it >= nint) return;
  const long f = blockIdx.y;
  const int hlen = (int)tab[kTabHeaderLen];
  uint8_t* file = out + offsets[f];
  if (it == 0) {
    const uint8_t* hdr = (const uint8_t*)(tab + kTabHeader);
    for (int i = threadIdx.x; i < hlen; i += 256) file[i] = hdr[i];
  }
  const uint8_t* src = (const uint8_t*)(raw + ((size_t)f * g.mcus_y + (size_t)it * rows_per) * g.row_words);
  const long nbytes = ((long)ibits[f * g.mcus_y + it] + 7) / 8;
  uint8_t* dst = file + hlen + ioff[f * g.mcus_y + it];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned carry = 0;                                                 // 0xFF bytes before this step
  for (long i0 = 0; i0 < nbytes; i0 += 256) {
    const long i = i0 + threadIdx.x;
    const int b = i < nbytes ? src[i] : 0;
    const uint64_t ff = __ballot(b == 255);
    const unsigned below = (unsigned)__popcll(ff & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_wave[wv] = (unsigned)__popcll(ff);
    __syncthreads();
    unsigned before = carry + below;
    for (int k = 0; k < wv; ++k) before += s_wave[k];
    if (i < nbytes) {
      dst[i + before] = (uint8_t)b;
      if (b == 255) dst[i + before + 1] = 0;
    }
    carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  }
  if (threadIdx.x == 0) {
    uint8_t* end = dst + nbytes + carry;
    end[0] = 0xFF;
    end[1] = it + 1 < nint ? (uint8_t)(0xD0 + (it & 7)) : (uint8_t)0xD9;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
const char* geometry_error(int H, int W) {
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return "H and W must be in 1..65535";
  if ((long)H * W > kMaxPixels) return "frame too large (H * W must not exceed 2^26)";
  return nullptr;
}

struct Layout {
  size_t coef, bbits, ibits, isize, fsize, raw, total;
};

Layout make_layout(int frames, const Geo& g) {
  Layout L;
  size_t at = 0;
  L.coef = at;
  at += align16((size_t)frames * g.nblk * 128);
  L.bbits = at;
  at += align16((size_t)frames * g.nblk * 4);
  L.ibits = at;
  at += align16((size_t)frames * g.mcus_y * 4);
  L.isize = at;
  at += align16((size_t)frames * g.mcus_y * 4);
  L.fsize = at;
  at += align16((size_t)frames * 8);
  L.raw = at;
  at += align16((size_t)frames * g.mcus_y * g.row_words * 4);
  L.total = at;
  return L;
}

struct Bytes {
  unsigned char* p;
  int n, cap;
  void put(int v) {
    if (n < cap) p[n] = (unsigned char)v;
    ++n;
  }
  void put16(int v) {
    put(v >> 8);
    put(v & 255);
  }
  void segment(int marker, int body) {
    put(0xFF);
    put(marker);
    put16(body + 2);
  }
};

void huffman_entries(const unsigned char* bits, const unsigned char* vals, uint32_t* entries) {
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) entries[vals[k++]] = (uint32_t)len << 16 | (uint32_t)code++;
    code <<= 1;
  }
}

void dht(Bytes& o, int tc_th, const unsigned char* bits, const unsigned char* vals, int n) {
  o.segment(0xC4, 17 + n);
  o.put(tc_th);
  for (int i = 0; i < 16; ++i) o.put(bits[i]);
  for (int i = 0; i < n; ++i) o.put(vals[i]);
}

}  // namespace

extern "C" int rmem_jpeg_encode_header(int H, int W, int quality, int restart_rows, unsigned char* header, int capacity,
                                       int* header_bytes, void* tables) {
  if (const char* why = geometry_error(H, W)) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "rmem_jpeg_encode_header: %s", why);
    rmem_set_error(msg);
    return -1;
  }
  RMEM_REQUIRE(quality >= 1 && quality <= 100, "rmem_jpeg_encode_header: quality must be in 1..100");
  const Geo g = make_geo(H, W);
  RMEM_REQUIRE(restart_rows >= 0 && (long)restart_rows * g.mcus_x <= 65535,
               "rmem_jpeg_encode_header: restart_rows * ceil(W / 16) must be in 0..65535 (the DRI field has 16 bits)");
  RMEM_REQUIRE(header_bytes, "rmem_jpeg_encode_header: null argument");
  RMEM_REQUIRE(capacity >= 0 && (header || capacity == 0), "rmem_jpeg_encode_header: bad header buffer");
  uint32_t tab[kTabWords];
  memset(tab, 0, sizeof tab);
  // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  int q[2][64];
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      q[t][i] = std::min(std::max(((t ? kQChroma : kQLuma)[i] * scale + 50) / 100, 1), 255);
      tab[kTabQ + t * 64 + i] = 8u * q[t][i];
    }
  huffman_entries(kDcLumaBits, kDcVals, tab + kTabDc);
  huffman_entries(kDcChromaBits, kDcVals, tab + kTabDc + 16);
  huffman_entries(kAcLumaBits, kAcLumaVals, tab + kTabAc);
  huffman_entries(kAcChromaBits, kAcChromaVals, tab + kTabAc + 256);
  Bytes o{(unsigned char*)(tab + kTabHeader), 0, (kTabWords - kTabHeader) * 4};
  o.put(0xFF);
  o.put(0xD8);
  o.segment(0xE0, 14);
  for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) o.put(v);   // "JFIF\0", 1.01, no density unit, 1:1, no thumbnail
  for (int t = 0; t < 2; ++t) {
    o.segment(0xDB, 65);
    o.put(t);
    for (int i = 0; i < 64; ++i) o.put(q[t][kZigzag[i]]);
  }
  o.segment(0xC0, 15);
  o.put(8);
  o.put16(H);
  o.put16(W);
  for (int v : {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) o.put(v);
  dht(o, 0x00, kDcLumaBits, kDcVals, 12);
  dht(o, 0x10, kAcLumaBits, kAcLumaVals, 162);
  dht(o, 0x01, kDcChromaBits, kDcVals, 12);
  dht(o, 0x11, kAcChromaBits, kAcChromaVals, 162);
  if (restart_rows) {
    o.segment(0xDD, 2);
    o.put16(restart_rows * g.mcus_x);
  }
  o.segment(0xDA, 10);
  for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) o.put(v);
  RMEM_REQUIRE(o.n <= RMEM_JPEG_ENC_HEADER_MAX && o.n <= o.cap, "rmem_jpeg_encode_header: internal error (header too long)");
  tab[kTabRestart] = (uint32_t)restart_rows;
  tab[kTabHeaderLen] = (uint32_t)o.n;
  tab[kTabH] = (uint32_t)H;
  tab[kTabW] = (uint32_t)W;
  *header_bytes = o.n;
  if (header) {
    RMEM_REQUIRE(capacity >= o.n, "rmem_jpeg_encode_header: header buffer too small (RMEM_JPEG_ENC_HEADER_MAX bytes always suffice)");
    memcpy(header, o.p, o.n);
  }
  if (tables) memcpy(tables, tab, sizeof tab);
  return 0;
}

// Most bytes one frame's file can take.  A block costs at most 22 + 63 * 26 bits = 208 bytes (DC: an 11-bit code and 11 value bits;
// every AC: a 16-bit code and 10 value bits), every byte of the scan may be 0xFF and grow a 0x00, every interval pads to a byte
// and is followed by a 2-byte marker, and a frame has at most one interval per MCU row; the header (with DRI) and EOI are fixed.
extern "C" size_t rmem_jpeg_encode_bound(int H, int W) {
  if (geometry_error(H, W)) return 0;
  const Geo g = make_geo(H, W);
  return (size_t)RMEM_JPEG_ENC_HEADER_MAX + 2 * ((size_t)g.nblk * kBlockBytes) + 4 * (size_t)g.mcus_y + 2;
}

extern "C" size_t rmem_jpeg_encode_workspace_bytes(int frames, int H, int W) {
  if (frames < 1 || geometry_error(H, W)) return 0;
  return make_layout(frames, make_geo(H, W)).total;
}

extern "C" int rmem_overlay_rgb8(const unsigned char* rgb, const unsigned char* labels, const unsigned char* palette, int alpha256,
                                 int frames, int H, int W, unsigned char* out_rgb, void* stream) {
  RMEM_REQUIRE(frames >= 1 && frames <= 65535 && H >= 1 && W >= 1, "rmem_overlay_rgb8: frames (at most 65535), H and W must be positive");
  RMEM_REQUIRE((long)H * W <= kMaxPixels, "rmem_overlay_rgb8: frame too large (H * W must not exceed 2^26)");
  RMEM_REQUIRE(alpha256 >= 0 && alpha256 <= 256, "rmem_overlay_rgb8: alpha256 must be in 0..256");
  RMEM_REQUIRE(rgb && labels && palette && out_rgb, "rmem_overlay_rgb8: null argument");
  const long hw = (long)H * W;
  const int blocks = (int)std::min<long>((hw + 255) / 256, 4096);
  hipLaunchKernelGGL(k_overlay, dim3(blocks, frames), dim3(256), 0, (hipStream_t)stream, rgb, labels, palette, alpha256, H, W, out_rgb);
  return rmem_check_launch("rmem_overlay_rgb8");
}

extern "C" int rmem_jpeg_encode_rgb8(const unsigned char* rgb, const unsigned char* labels, const unsigned char* palette, int alpha256,
                                     int frames, int H, int W, const void* tables, void* workspace, unsigned char* out,
                                     long long* offsets, void* stream) {
  RMEM_REQUIRE(frames >= 1 && frames <= 65535, "rmem_jpeg_encode_rgb8: frames must be in 1..65535");
  if (const char* why = geometry_error(H, W)) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "rmem_jpeg_encode_rgb8: %s", why);
    rmem_set_error(msg);
    return -1;
  }
  RMEM_REQUIRE(rgb && tables && workspace && out && offsets, "rmem_jpeg_encode_rgb8: null argument");
  RMEM_REQUIRE(!labels || palette, "rmem_jpeg_encode_rgb8: null argument (labels without a palette)");
  RMEM_REQUIRE(!labels || (alpha256 >= 0 && alpha256 <= 256), "rmem_jpeg_encode_rgb8: alpha256 must be in 0..256");
  RMEM_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tables & 3) == 0,
               "rmem_jpeg_encode_rgb8: workspace must be 16-byte aligned and tables 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Geo g = make_geo(H, W);
  const Layout L = make_layout(frames, g);
  uint8_t* ws = (uint8_t*)workspace;
  int16_t* coef = (int16_t*)(ws + L.coef);
  uint32_t* bbits = (uint32_t*)(ws + L.bbits);
  uint32_t* ibits = (uint32_t*)(ws + L.ibits);
  uint32_t* isize = (uint32_t*)(ws + L.isize);
  unsigned long long* fsize = (unsigned long long*)(ws + L.fsize);
  uint32_t* raw = (uint32_t*)(ws + L.raw);
  const uint32_t* tab = (const uint32_t*)tables;
  const int strips = (g.mcus + kMcusPerGroup - 1) / kMcusPerGroup;
  const int block_groups = (int)std::min<long>((g.nblk + 255) / 256, 65535);
  hipLaunchKernelGGL(k_jenc_mcu, dim3(strips, frames), dim3(256), 0, st, rgb, labels, palette, alpha256, g, tab, coef);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (mcu)")) return rc;
  hipLaunchKernelGGL(k_jenc_size, dim3(block_groups, frames), dim3(256), 0, st, coef, g, tab, bbits);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (size)")) return rc;
  hipLaunchKernelGGL(k_jenc_scan, dim3(g.mcus_y, frames), dim3(256), 0, st, bbits, g, tab, ibits, raw);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (scan)")) return rc;
  hipLaunchKernelGGL(k_jenc_emit, dim3(block_groups, frames), dim3(256), 0, st, coef, g, tab, bbits, ibits, raw);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (emit)")) return rc;
  hipLaunchKernelGGL(k_jenc_count, dim3(g.mcus_y, frames), dim3(256), 0, st, g, tab, ibits, raw, isize);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (count)")) return rc;
  hipLaunchKernelGGL(k_jenc_frames, dim3(frames), dim3(256), 0, st, g, tab, isize, fsize);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (frames)")) return rc;
  hipLaunchKernelGGL(k_codec_offsets, dim3(1), dim3(256), 0, st, fsize, frames, offsets);
  if (int rc = rmem_check_launch("rmem_jpeg_encode_rgb8 (offsets)")) return rc;
  hipLaunchKernelGGL(k_jenc_place, dim3(g.mcus_y, frames), dim3(256), 0, st, g, tab, ibits, isize, raw, offsets, out);
  return rmem_check_launch("rmem_jpeg_encode_rgb8 (place)");
}
