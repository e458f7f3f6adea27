// Palette-PNG payloads on the device (include/rmem.h, rmem_png_*): one zlib stream per uint8 label map, packed back to back.
//
// The stream is fixed bit for bit (include/rmem.h): 78 01, one fixed-Huffman DEFLATE block over the "Up"-filtered rows, every
// row cut into maximal runs of equal bytes, a run = literal, distance-1 matches of up to 258, at most two closing literals.
// Nothing in it needs a table built from the data, so the encoder is count bits, scan, emit:
//   k_png_count   one wave per row, 64 filtered bytes per step (lane = byte).  A ballot of `byte != previous byte` gives the run
//                 starts; the lane on which a run ENDS (the next run's start, or the position one past the row) knows the run's
//                 value and, from the ballot's next lower bit or the length carried over from earlier steps, its length, and
//                 prices it in closed form.  Writes bits[f][y] and the row's Adler-32 partials s1 = sum b_j,
//                 s2 = sum (W + 1 - j) b_j, both mod 65521 (accumulated in 64 bits).
//   k_png_rows    one workgroup per frame: exclusive scan of the row bits (in place), the frame's byte size, and its Adler-32
//                 A = 1 + sum s1_y, B = H (W + 1) + sum (s2_y + (H - 1 - y)(W + 1) s1_y)  (mod 65521) -- the row combine
//                 A' = A + s1, B' = B + len A + s2 unrolled, so it is a plain sum.
//   k_codec_offsets (codec.h) one workgroup: exclusive scan of the frame sizes -> offsets[0..frames].
//   k_png_zero    zeroes the words of out[0 : offsets[frames]) -- the bytes this call uses, not the whole bound.
//   k_png_emit    k_png_count's pass again (the labels are read a second time instead of keeping a per-row scratch of the
//                 bound's size); every run-ending lane gets its bit position from a wave scan and writes its run's tokens through
//                 a 64-bit accumulator, one 32-bit word at a time.  Ownership rule: a word that lies wholly inside one run's bits
//                 is a plain store; a word shared with a neighbouring run, row, header or frame is OR-ed into the zeroed memory
//                 with a vector atomic.  The wave of row 0 also writes the 19 header bits, the wave of the last row the
//                 Adler-32 (end-of-block and padding are zero bits: nothing to write).
// The words are 32-bit words of `out` (4-byte aligned).  The last word of the last frame may reach past offsets[frames]; its
// bytes inside belong to the Adler-32 alone and are stored as bytes, so nothing is touched beyond out + frames * bound.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "common.h"
#include "codec.h"
#include "../../include/rmem.h"

namespace {

constexpr unsigned kAdler = 65521u;
constexpr int kHeaderBits = 19;         // 78 01, BFINAL = 1, BTYPE = 01

__device__ __forceinline__ int lit_bits(int v) { return v < 144 ? 8 : 9; }

// the length symbol of a match of length t in 3..257: Huffman code length, number of extra bits, symbol
__device__ __forceinline__ void len_symbol(int t, int& sym, int& clen, int& extra) {
  const int m = t - 3;
  extra = m < 8 ? 0 : 29 - __builtin_clz(m);
  sym = 257 + 4 * extra + (m >> extra);
  clen = sym < 280 ? 7 : 8;
}

// bits of one run: literal, k = rem / 258 matches of 258 (13 bits each), then a match of r = rem % 258 >= 3 or r literals
__device__ __forceinline__ unsigned run_bits(int v, int L) {
  const int rem = L - 1, k = rem / 258, r = rem - k * 258;
  unsigned bits = lit_bits(v) + 13u * k;
  if (r >= 3) {
    int sym, clen, extra;
    len_symbol(r, sym, clen, extra);
    bits += clen + extra + 5;
  } else {
    bits += r * lit_bits(v);
  }
  return bits;
}

// LSB-first bit writer of one lane: see the ownership rule above
struct BitWriter {
  uint32_t* w;
  uint64_t acc;
  int nb;
  bool shared;
  __device__ __forceinline__ BitWriter(uint32_t* words, uint64_t bitpos) : w(words + (bitpos >> 5)), acc(0), nb((int)(bitpos & 31)) {
    shared = nb != 0;
  }
  __device__ __forceinline__ void put(uint32_t code, int len) {      // len <= 18
    acc |= (uint64_t)code << nb;
    nb += len;
    if (nb >= 32) {
      const uint32_t x = (uint32_t)acc;
      if (shared) {
        if (x) atomicOr(w, x);
      } else {
        *w = x;
      }
      shared = false;
      ++w;
      acc >>= 32;
      nb -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nb > 0 && (uint32_t)acc) atomicOr(w, (uint32_t)acc);
  }
};

__device__ __forceinline__ uint32_t lit_code(int v) {                // Huffman codes go out most significant bit first
  return v < 144 ? __brev(0x30u + v) >> 24 : __brev(0x190u + (v - 144)) >> 23;
}

__device__ __forceinline__ void put_run(BitWriter& bw, int v, int L) {
  const uint32_t lc = lit_code(v);
  const int lb = lit_bits(v);
  bw.put(lc, lb);
  const int rem = L - 1, k = rem / 258, r = rem - k * 258;
  for (int i = 0; i < k; ++i) bw.put(0xA3u, 13);                     // symbol 285 = 11000101 reversed, distance code 0
  if (r >= 3) {
    int sym, clen, extra;
    len_symbol(r, sym, clen, extra);
    const uint32_t code = sym < 280 ? __brev((uint32_t)(sym - 256)) >> 25 : __brev(0xC0u + (sym - 280)) >> 24;
    const uint32_t ev = (uint32_t)(r - 3) & ((1u << extra) - 1u);
    bw.put(code | ev << clen, clen + extra + 5);
  } else {
    for (int i = 0; i < r; ++i) bw.put(lc, lb);
  }
}

// One row by one wave.  Filtered byte j of the row (0 <= j <= W): j = 0 is the filter type 2, else lut[cur[j-1]] - lut[up[j-1]].
// Position W + 1 ends the last run.  EMIT = false: returns the row's bits, s1 and s2 in 64 bits per lane (not yet reduced).
template <bool EMIT>
__device__ __forceinline__ unsigned row_pass(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ up, const uint8_t* lut, int W,
                                             int lane, uint64_t& s1, uint64_t& s2, uint32_t* words, uint64_t bitpos) {
  unsigned row_bits = 0;
  int open_len = 0;           // bytes of the run that is open at the start of this step (wave-uniform)
  int last = 0;               // the filtered byte before this step's first one (wave-uniform)
  const uint64_t below = (1ull << lane) - 1ull;
  int nc = 0, nu = 0;
  if (lane >= 1 && lane <= W) {
    nc = cur[lane - 1];
    nu = up ? up[lane - 1] : 0;
  }
  for (int j0 = 0; j0 <= W + 1; j0 += 64) {
    const int j = j0 + lane;
    const int c = nc, u = nu;
    const int jn = j + 64;                                            // the next step's labels are requested before this one's work
    if (jn <= W) {
      nc = cur[jn - 1];
      nu = up ? up[jn - 1] : 0;
    }
    int b = 0;
    if (j == 0) b = 2;
    else if (j <= W) b = ((int)lut[c] - (up ? (int)lut[u] : 0)) & 255;
    int pb = __shfl_up(b, 1, 64);
    if (lane == 0) pb = last;
    const bool start = j <= W + 1 && (j == 0 || j == W + 1 || b != pb);
    const uint64_t mask = __ballot(start);
    const bool ends = start && j > 0;                                 // this lane closes the run of value pb that ends at j - 1
    int L = 0;
    unsigned bits = 0;
    if (ends) {
      const uint64_t lower = mask & below;
      L = lower ? lane - (63 - __builtin_clzll(lower)) : open_len + lane;
      bits = run_bits(pb, L);
    }
    const unsigned incl = wave_incl_scan(bits);
    if (EMIT) {
      if (ends) {
        BitWriter bw(words, bitpos + row_bits + (incl - bits));
        put_run(bw, pb, L);
        bw.finish();
      }
    } else if (j <= W) {
      s1 += (unsigned)b;
      s2 += (uint64_t)(W + 1 - j) * (unsigned)b;
    }
    row_bits += __shfl(incl, 63, 64);
    open_len = mask ? __builtin_clzll(mask) + 1 : open_len + 64;
    last = __shfl(b, 63, 64);
  }
  return row_bits;
}

__device__ __forceinline__ void load_lut(uint8_t* s_lut, const uint8_t* lut) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = lut ? lut[i] : (uint8_t)i;
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_png_count(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ lut, long rows, int H,
                                                   int W, uint32_t* __restrict__ bits, uint32_t* __restrict__ a1, uint32_t* __restrict__ a2) {
  __shared__ uint8_t s_lut[256];
  load_lut(s_lut, lut);
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
    const int y = (int)(r % H);
    const uint8_t* cur = labels + r * W;
    uint64_t s1 = 0, s2 = 0;
    const unsigned nbits = row_pass<false>(cur, y ? cur - W : nullptr, s_lut, W, lane, s1, s2, nullptr, 0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    if (lane == 0) {
      bits[r] = nbits;
      a1[r] = (uint32_t)(s1 % kAdler);
      a2[r] = (uint32_t)(s2 % kAdler);
    }
  }
}

// bytes of a frame whose rows take `bits` bits: header, block header + tokens + end-of-block padded to a byte, Adler-32
__host__ __device__ __forceinline__ uint64_t frame_bytes(uint64_t bits) { return 2 + (3 + bits + 7 + 7) / 8 + 4; }

__global__ __launch_bounds__(256) void k_png_rows(uint32_t* __restrict__ bits, const uint32_t* __restrict__ a1, const uint32_t* __restrict__ a2,
                                                  int H, int W, uint32_t* __restrict__ adler, unsigned long long* __restrict__ sizes) {
  __shared__ unsigned s_wave[4];
  __shared__ unsigned long long s_red[2][4];
  const int f = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* const fb = bits + (long)f * H;
  const uint32_t* const f1 = a1 + (long)f * H;
  const uint32_t* const f2 = a2 + (long)f * H;
  const uint64_t len = (uint64_t)W + 1;
  unsigned carry = 0;
  uint64_t A = 0, B = 0;                                              // per thread, reduced below: at most H terms below 2^16 * 2^16 each
  for (int y0 = 0; y0 < H; y0 += 256) {
    const int y = y0 + threadIdx.x;
    const unsigned at = block_excl_scan(y < H ? fb[y] : 0u, s_wave, carry);
    if (y < H) {
      fb[y] = at;
      A += f1[y];
      B += (f2[y] + ((uint64_t)(H - 1 - y) * len % kAdler) * f1[y]) % kAdler;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    A += __shfl_xor(A, o, 64);
    B += __shfl_xor(B, o, 64);
  }
  if (lane == 0) {
    s_red[0][wv] = A;
    s_red[1][wv] = B;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t a = (1 + s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]) % kAdler;
    const uint64_t b = ((uint64_t)H * len + s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3]) % kAdler;
    adler[f] = (uint32_t)(b << 16 | a);
    sizes[f] = frame_bytes(carry);
  }
}

__global__ __launch_bounds__(256) void k_png_zero(uint32_t* __restrict__ words, const long long* __restrict__ offsets, int frames) {
  const long n = offsets[frames] >> 2;                                // whole words; the last partial one is stored as bytes
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) words[i] = 0;
}

__global__ __launch_bounds__(256) void k_png_emit(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ lut, long rows, int H, int W,
                                                  int frames, const uint32_t* __restrict__ bits, const uint32_t* __restrict__ adler,
                                                  const long long* __restrict__ offsets, uint8_t* __restrict__ out) {
  __shared__ uint8_t s_lut[256];
  load_lut(s_lut, lut);
  const int lane = threadIdx.x & 63;
  uint32_t* const words = (uint32_t*)out;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
    const int f = (int)(r / H), y = (int)(r - (long)f * H);
    const uint8_t* cur = labels + r * W;
    const uint64_t base = (uint64_t)offsets[f] * 8;
    uint64_t s1 = 0, s2 = 0;
    row_pass<true>(cur, y ? cur - W : nullptr, s_lut, W, lane, s1, s2, words, base + kHeaderBits + bits[r]);
    if (y == 0 && lane == 0) {
      BitWriter bw(words, base);
      bw.put(0x0178u, 16);
      bw.put(3u, 3);
      bw.finish();
    }
    if (y == H - 1 && lane == 0) {                                    // Adler-32, big-endian, in the frame's last four bytes
      const uint32_t a = adler[f];
      const uint64_t end = (uint64_t)offsets[f + 1];
      const uint64_t tail_word = (uint64_t)offsets[frames] >> 2;      // whole words end here
      for (int i = 0; i < 4; ++i) {
        const uint64_t at = end - 4 + i;
        const uint32_t byte = (a >> (24 - 8 * i)) & 255u;
        if ((at >> 2) >= tail_word) out[at] = (uint8_t)byte;          // never zeroed, never shared: see the head of this file
        else if (byte) atomicOr(words + (at >> 2), byte << (8 * (at & 3)));
      }
    }
  }
}

}  // namespace

extern "C" size_t rmem_png_zlib_bound(int H, int W) {
  if (!geometry_ok(1, H, W)) return 0;
  return (size_t)frame_bytes(9ull * ((uint64_t)W + 1) * (uint64_t)H);
}

extern "C" size_t rmem_png_workspace_bytes(int frames, int H, int W) {
  if (!geometry_ok(frames, H, W)) return 0;
  // bits, s1, s2: uint32 [frames][H]; Adler-32: uint32 [frames]; frame sizes: uint64 [frames]
  return 3 * align16((size_t)frames * H * 4) + align16((size_t)frames * 4) + align16((size_t)frames * 8);
}

extern "C" int rmem_png_encode_labels(const unsigned char* labels, int frames, int H, int W, const unsigned char* lut, void* workspace,
                                      unsigned char* out, long long* offsets, void* stream) {
  RMEM_REQUIRE(frames >= 1 && H >= 1 && W >= 1, "rmem_png_encode_labels: frames, H and W must be positive");
  RMEM_REQUIRE((long)H * W <= kMaxPixels, "rmem_png_encode_labels: frame too large (H * W must not exceed 2^26)");
  RMEM_REQUIRE(labels && workspace && out && offsets, "rmem_png_encode_labels: null argument");
  RMEM_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
               "rmem_png_encode_labels: out must be 4-byte aligned and workspace 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long rows = (long)frames * H;
  const size_t plane = align16((size_t)rows * 4);
  uint8_t* ws = (uint8_t*)workspace;
  uint32_t* bits = (uint32_t*)ws;
  uint32_t* a1 = (uint32_t*)(ws + plane);
  uint32_t* a2 = (uint32_t*)(ws + 2 * plane);
  uint32_t* adler = (uint32_t*)(ws + 3 * plane);
  unsigned long long* sizes = (unsigned long long*)(ws + 3 * plane + align16((size_t)frames * 4));
  const int row_blocks = (int)std::min((rows + 3) / 4, 1L << 20);
  hipLaunchKernelGGL(k_png_count, dim3(row_blocks), dim3(256), 0, st, labels, lut, rows, H, W, bits, a1, a2);
  if (int rc = rmem_check_launch("rmem_png_encode_labels (count)")) return rc;
  hipLaunchKernelGGL(k_png_rows, dim3(frames), dim3(256), 0, st, bits, a1, a2, H, W, adler, sizes);
  if (int rc = rmem_check_launch("rmem_png_encode_labels (rows)")) return rc;
  hipLaunchKernelGGL(k_codec_offsets, dim3(1), dim3(256), 0, st, sizes, frames, offsets);
  if (int rc = rmem_check_launch("rmem_png_encode_labels (frames)")) return rc;
  const size_t bound_words = (size_t)frames * rmem_png_zlib_bound(H, W) / 4;
  const int zero_blocks = (int)std::min<size_t>(std::max<size_t>((bound_words / 64 + 255) / 256, 1), 2048);   // typical streams are 2-3 % of it
  hipLaunchKernelGGL(k_png_zero, dim3(zero_blocks), dim3(256), 0, st, (uint32_t*)out, offsets, frames);
  if (int rc = rmem_check_launch("rmem_png_encode_labels (zero)")) return rc;
  hipLaunchKernelGGL(k_png_emit, dim3(row_blocks), dim3(256), 0, st, labels, lut, rows, H, W, frames, bits, adler, offsets, out);
  return rmem_check_launch("rmem_png_encode_labels (emit)");
}
