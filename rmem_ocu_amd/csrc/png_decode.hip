// Palette-PNG annotations on the device (include/rmem.h, rmem_png_decode_*): zlib streams in, uint8 label maps out.
//
//   k_pngd_inflate   one wavefront (one 64-thread workgroup) per stream.  DEFLATE's symbol stream is serial, so everything that
//                    steers it -- the bit position, the block state, the output position, the status -- is wave-uniform C++; the
//                    lanes work in parallel where the format allows it:
//                      * the canonical Huffman tables of a block (count per length with LDS atomics, the symbols ranked in code
//                        order with one ballot per length, the 10-bit primary table filled 16 entries per lane by walking the
//                        canonical code); codes longer than 10 bits, which a primary entry of 0 marks, walk the same canonical
//                        arrays for lengths 11..15 (the second level);
//                      * literals are collected one per lane and stored up to 64 at a time;
//                      * a match is copied by all lanes: for distance d < 64 the pattern byte of lane l, ring[pos - d + l mod d],
//                        is read ONCE and written P = d * floor(64 / d) bytes per step (no read depends on a write of the same
//                        match); for d >= 64 a step reads 64 bytes that lie wholly below the bytes it writes.
//                    Back-references read an LDS ring of the last 32 KiB of output: LDS operations of one wave complete in order,
//                    and a read costs tens of cycles where a global round trip costs hundreds, on the one path that is serial.
//                    Every byte goes to the ring and to the workspace (the filtered bytes of the frame).  The Adler-32 is
//                    accumulated per lane in closed form, A = 1 + sum b_j, B = N + sum (N - j) b_j (j from 0, N = H * stride),
//                    reduced once at the end and compared with the trailer.
//   k_pngd_unfilter  grid (row slabs, frames), 256 threads.  Every block scans the frame's H filter bytes.  All zero (what Pillow
//                    writes for 8-bit palette maps): the rows are independent and every slab does its own.  Otherwise slab 0
//                    walks the rows in order, reconstructing them in place in the workspace: None / Up per byte, Sub as a
//                    block-wide prefix sum mod 256, Average / Paeth by one thread from LDS.  Then the samples are unpacked
//                    (most significant bits first, a row's padding bits ignored) and go through the 256-entry table.  A frame
//                    whose status is not zero is zero-filled, so `out` never keeps stale bytes.
//
// Bounds.  Input: BitReader::word / byte are the only reads of the compressed bytes; beyond `nbytes` they return zero without
// touching memory, and consuming past nbytes * 8 bits raises ST_INPUT and ends the stream.  Output: Sink::put is the only write
// and is reached only after `pos + n <= N` was checked (else ST_SIZE).  Back-references: distance <= pos is checked (else
// ST_RANGE); ring indices are masked.  Every loop iteration of the decoder consumes at least one input bit or ends the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "common.h"
#include "codec.h"
#include "../../include/rmem.h"

namespace {

constexpr unsigned kRing = 32768u;      // DEFLATE's largest distance
constexpr unsigned kAdler = 65521u;
constexpr int kTabBits = 10;            // primary table of the literal/length and the distance code
constexpr int kClBits = 7;              // the code-length code has no longer codes
constexpr int kMaxLens = 320;           // 286 + 30 code lengths of a dynamic block, 288 + 32 of the fixed one

enum { KIND_CL = 0, KIND_LIT = 1, KIND_DIST = 2 };
enum { TABLES_NONE = 0, TABLES_FIXED = 1, TABLES_DYNAMIC = 2 };

__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Huff {                           // one canonical code, in LDS
  uint16_t primary[1 << kTabBits];      // index: the next bits as they come; entry: symbol << 4 | length, 0 = not a code of <= TB bits
  uint16_t sorted[kMaxLens];            // the symbols in code order
  int cnt[16], first[16], offs[16];     // per length: codes, the first code, its index in sorted
};

struct Shared {
  uint8_t ring[kRing];
  Huff lit, dist;                       // dist also holds the code-length code while a dynamic header is read
  uint8_t lens[kMaxLens];
  uint8_t cl_lens[32];
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The only reader of the compressed bytes of one stream (wave-uniform state).
struct BitReader {
  const uint8_t* base;                  // 8-byte aligned
  uint64_t nbytes;
  uint64_t bitpos;                      // bits consumed
  uint64_t w0, w1;                      // words wi and wi + 1
  uint64_t wi;
  __device__ __forceinline__ uint64_t word(uint64_t k) const {
    const uint64_t b = k * 8;
    if (b >= nbytes) return 0;
    uint64_t v = *(const uint64_t*)(base + b);          // a stream is padded to a whole word: include/rmem.h
    const uint64_t rem = nbytes - b;
    if (rem < 8) v &= (1ull << (8 * rem)) - 1ull;
    return v;
  }
  __device__ __forceinline__ unsigned byte(uint64_t i) const { return i < nbytes ? base[i] : 0u; }
  __device__ __forceinline__ void init(const uint8_t* p, uint64_t n) {
    base = p;
    nbytes = n;
    bitpos = 0;
    wi = 0;
    w0 = word(0);
    w1 = word(1);
  }
  __device__ __forceinline__ uint64_t peek() {          // the next 64 bits, least significant first
    const uint64_t k = bitpos >> 6;
    if (k != wi) {
      w0 = k == wi + 1 ? w1 : word(k);
      w1 = word(k + 1);
      wi = k;
    }
    const int sh = (int)(bitpos & 63);
    return sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
  }
  __device__ __forceinline__ void skip(int n) { bitpos += (unsigned)n; }
  __device__ __forceinline__ bool overrun() const { return bitpos > nbytes * 8; }
  // no code matches the next 15 bits: an invalid code, unless fewer than 15 bits are left and the zeros behind them were read
  __device__ __forceinline__ unsigned bad_code() const { return bitpos + 15 > nbytes * 8 ? RMEM_PNG_ST_INPUT : RMEM_PNG_ST_CODE; }
};

// The only writer of the inflated bytes: the LDS ring, the workspace, the Adler-32 sums.
struct Sink {
  uint8_t* dst;
  uint8_t* ring;
  uint32_t N, pos;                      // wave-uniform
  uint64_t s1, s2;                      // per lane
  unsigned pend;                        // per lane: the literal waiting in this lane
  int npend;                            // wave-uniform
  __device__ __forceinline__ void put(uint32_t p, unsigned b) {       // the caller has checked p < N
    ring[p & (kRing - 1)] = (uint8_t)b;
    dst[p] = (uint8_t)b;
    s1 += b;
    s2 += (uint64_t)(N - p) * b;
  }
  __device__ __forceinline__ unsigned flush(int lane) {
    if (npend == 0) return 0;
    if (pos + (uint32_t)npend > N) return RMEM_PNG_ST_SIZE;
    if (lane < npend) put(pos + lane, pend);
    pos += npend;
    npend = 0;
    return 0;
  }
  __device__ __forceinline__ unsigned literal(int v, int lane) {
    if (lane == npend) pend = (unsigned)v;
    if (++npend == 64) return flush(lane);
    return 0;
  }
};

// symbol and length of the code at the head of `b` (TB = bits of h's primary table); false: no such code
template <int TB>
__device__ __forceinline__ bool decode(const Huff& h, uint64_t b, int& sym, int& len) {
  const int e = uni(h.primary[(unsigned)b & ((1u << TB) - 1u)]);
  if (e & 15) {
    sym = e >> 4;
    len = e & 15;
    return true;
  }
  const unsigned rev = __brev((unsigned)b) >> 17;       // the next 15 bits, first bit on top: Huffman codes come most significant bit first
  for (int l = TB + 1; l <= 15; ++l) {
    const unsigned d = (rev >> (15 - l)) - (unsigned)uni(h.first[l]);
    if (d < (unsigned)uni(h.cnt[l])) {
      sym = uni(h.sorted[uni(h.offs[l]) + d]);
      len = l;
      return true;
    }
  }
  return false;
}

// Canonical code of the n lengths lens[0..n) into h.  Over-subscribed: ST_CODE.  Incomplete: ST_CODE unless it is a single code of
// one bit (zlib's rule for the literal/length and distance codes; the code-length code must be complete) or no code at all (an
// all-literal block's distance code; using it is then an invalid code).
template <int TB>
__device__ unsigned build_table(Huff& h, const uint8_t* lens, int n, int kind, int lane) {
  __syncthreads();
  if (lane < 16) h.cnt[lane] = 0;
  __syncthreads();
  for (int s = lane; s < n; s += 64) {
    const int l = lens[s];
    if (l) atomicAdd(&h.cnt[l], 1);
  }
  __syncthreads();
  int left = 1, code = 0, off = 0, maxlen = 0;
  for (int l = 1; l <= 15; ++l) {
    const int c = uni(h.cnt[l]);
    code <<= 1;
    left = left * 2 - c;
    if (left < 0) return RMEM_PNG_ST_CODE;
    if (lane == 0) {
      h.first[l] = code;
      h.offs[l] = off;
    }
    code += c;
    off += c;
    if (c) maxlen = l;
  }
  if (left > 0 && off > 0 && (kind == KIND_CL || maxlen != 1)) return RMEM_PNG_ST_CODE;
  __syncthreads();
  // rank the symbols in code order: by length, then by symbol.  Lane l < 16 carries the next free index of length l.
  int next = lane >= 1 && lane < 16 ? h.offs[lane] : 0;
  const uint64_t below = (1ull << lane) - 1ull;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int s = s0 + lane;
    const int l = s < n ? lens[s] : 0;
    for (int len = 1; len <= maxlen; ++len) {
      const uint64_t m = __ballot(l == len);
      if (m == 0) continue;
      const int at = __shfl(next, len, 64);
      if (l == len) h.sorted[at + __builtin_popcountll(m & below)] = (uint16_t)s;
      if (lane == len) next += __builtin_popcountll(m);
    }
  }
  __syncthreads();
  int fi[TB + 1], cn[TB + 1], of[TB + 1];
#pragma unroll
  for (int l = 1; l <= TB; ++l) {
    fi[l] = uni(h.first[l]);
    cn[l] = uni(h.cnt[l]);
    of[l] = uni(h.offs[l]);
  }
  for (int e = lane; e < (1 << TB); e += 64) {
    const unsigned rev = __brev((unsigned)e) >> (32 - TB);
    unsigned entry = 0;
#pragma unroll
    for (int l = TB; l >= 1; --l) {                     // a prefix code: at most one length matches
      const unsigned d = (rev >> (TB - l)) - (unsigned)fi[l];
      if (d < (unsigned)cn[l]) entry = (unsigned)h.sorted[of[l] + d] << 4 | (unsigned)l;
    }
    h.primary[e] = (uint16_t)entry;
  }
  __syncthreads();
  return 0;
}

__device__ unsigned build_fixed(Shared& sm, int lane) {
  __syncthreads();
  for (int s = lane; s < 288; s += 64) sm.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
  if (lane < 32) sm.lens[288 + lane] = 5;
  __syncthreads();
  unsigned st = build_table<kTabBits>(sm.lit, sm.lens, 288, KIND_LIT, lane);
  if (!st) st = build_table<kTabBits>(sm.dist, sm.lens + 288, 32, KIND_DIST, lane);
  return st;
}

// the header of a dynamic block: HLIT, HDIST, HCLEN, the code-length code, then the HLIT + HDIST lengths as ONE sequence
__device__ unsigned read_dynamic(Shared& sm, BitReader& br, int lane) {
  uint64_t v = br.peek();
  const int hlit = (int)(v & 31) + 257, hdist = (int)(v >> 5 & 31) + 1, hclen = (int)(v >> 10 & 15) + 4;
  br.skip(14);
  if (hlit > 286 || hdist > 30) return RMEM_PNG_ST_CODE;
  v = br.peek();                                        // 19 * 3 = 57 bits
  __syncthreads();
  if (lane < 19) sm.cl_lens[lane] = 0;
  __syncthreads();
  if (lane < hclen) sm.cl_lens[kClOrder[lane]] = (uint8_t)(v >> (3 * lane) & 7);
  br.skip(3 * hclen);
  if (br.overrun()) return RMEM_PNG_ST_INPUT;
  __syncthreads();
  if (unsigned st = build_table<kClBits>(sm.dist, sm.cl_lens, 19, KIND_CL, lane)) return st;
  const int total = hlit + hdist;
  int i = 0, prev = 0;
  while (i < total) {
    v = br.peek();
    int sym, len;
    if (!decode<kClBits>(sm.dist, v, sym, len)) return br.bad_code();
    int rep = 1, val = sym;
    if (sym < 16) {
      br.skip(len);
    } else if (sym == 16) {
      if (i == 0) return RMEM_PNG_ST_CODE;
      rep = 3 + (int)(v >> len & 3);
      val = prev;
      br.skip(len + 2);
    } else if (sym == 17) {
      rep = 3 + (int)(v >> len & 7);
      val = 0;
      br.skip(len + 3);
    } else {
      rep = 11 + (int)(v >> len & 127);
      val = 0;
      br.skip(len + 7);
    }
    if (br.overrun()) return RMEM_PNG_ST_INPUT;
    if (i + rep > total) return RMEM_PNG_ST_CODE;
    for (int k = lane; k < rep; k += 64) sm.lens[i + k] = (uint8_t)val;
    i += rep;
    prev = val;
  }
  __syncthreads();
  if (uni(sm.lens[256]) == 0) return RMEM_PNG_ST_CODE;  // no end-of-block code
  if (unsigned st = build_table<kTabBits>(sm.lit, sm.lens, hlit, KIND_LIT, lane)) return st;
  return build_table<kTabBits>(sm.dist, sm.lens + hlit, hdist, KIND_DIST, lane);
}

// a stored block; the reader stands behind the block header
__device__ unsigned copy_stored(BitReader& br, Sink& out, int lane) {
  br.bitpos = (br.bitpos + 7) & ~7ull;
  const uint64_t v = br.peek();
  const unsigned len = (unsigned)v & 0xFFFFu, nlen = (unsigned)(v >> 16) & 0xFFFFu;
  br.skip(32);
  if (br.overrun()) return RMEM_PNG_ST_INPUT;
  if (len != (~nlen & 0xFFFFu)) return RMEM_PNG_ST_CODE;
  const uint64_t at = br.bitpos >> 3;
  if (at + len > br.nbytes) return RMEM_PNG_ST_INPUT;
  if (out.pos + len > out.N) return RMEM_PNG_ST_SIZE;
  for (unsigned k = 0; k < len; k += 64) {
    const unsigned i = k + lane;
    if (i < len) out.put(out.pos + i, br.byte(at + i));
  }
  out.pos += len;
  br.bitpos += 8ull * len;
  return 0;
}

// a match of `len` bytes `dist` back; pending literals are flushed, dist <= pos and pos + len <= N are checked
__device__ __forceinline__ void copy_match(Sink& out, unsigned len, unsigned dist, int lane) {
  __syncthreads();                                      // the ring writes before this point, seen by every lane
  const uint32_t pos = out.pos;
  if (dist < 64) {
    const unsigned P = dist * (64u / dist);
    const unsigned b = out.ring[(pos - dist + (unsigned)lane % dist) & (kRing - 1)];
    __syncthreads();
    for (unsigned k = 0; k < len; k += P) {
      const unsigned i = k + lane;
      if ((unsigned)lane < P && i < len) out.put(pos + i, b);
    }
  } else {
    for (unsigned k = 0; k < len; k += 64) {
      const unsigned i = k + lane;
      unsigned b = 0;
      if (i < len) b = out.ring[(pos - dist + i) & (kRing - 1)];
      __syncthreads();
      if (i < len) out.put(pos + i, b);
      __syncthreads();
    }
  }
  out.pos = pos + len;
}

__device__ unsigned inflate_stream(Shared& sm, BitReader& br, Sink& out, int lane) {
  uint64_t v = br.peek();                               // zlib header: CMF, FLG
  const unsigned cmf = (unsigned)v & 255u, flg = (unsigned)(v >> 8) & 255u;
  br.skip(16);
  if (br.overrun()) return RMEM_PNG_ST_INPUT;
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (cmf * 256u + flg) % 31u != 0u || (flg & 32u)) return RMEM_PNG_ST_HEADER;
  int tables = TABLES_NONE;
  bool last = false;
  while (!last) {
    v = br.peek();
    last = v & 1;
    const int btype = (int)(v >> 1 & 3);
    br.skip(3);
    if (br.overrun()) return RMEM_PNG_ST_INPUT;
    if (btype == 3) return RMEM_PNG_ST_CODE;
    if (btype == 0) {
      if (unsigned st = out.flush(lane)) return st;
      if (unsigned st = copy_stored(br, out, lane)) return st;
      continue;
    }
    if (btype == 1) {
      if (tables != TABLES_FIXED)
        if (unsigned st = build_fixed(sm, lane)) return st;
      tables = TABLES_FIXED;
    } else {
      tables = TABLES_NONE;
      if (unsigned st = read_dynamic(sm, br, lane)) return st;
      tables = TABLES_DYNAMIC;
    }
    for (;;) {                                          // one token per turn; a turn consumes at least one bit
      v = br.peek();
      int sym, n;
      if (!decode<kTabBits>(sm.lit, v, sym, n)) return br.bad_code();
      if (sym < 256) {
        br.skip(n);
        if (br.overrun()) return RMEM_PNG_ST_INPUT;
        if (unsigned st = out.literal(sym, lane)) return st;
        continue;
      }
      if (sym == 256) {
        br.skip(n);
        if (br.overrun()) return RMEM_PNG_ST_INPUT;
        break;
      }
      if (sym > 285) return RMEM_PNG_ST_CODE;
      v >>= n;
      int used = n;
      const int li = sym - 257;
      const int le = li < 8 || li == 28 ? 0 : (li - 4) >> 2;
      const unsigned len = (li == 28 ? 258u : li < 8 ? 3u + li : 3u + ((4u + (li & 3)) << le)) + ((unsigned)v & ((1u << le) - 1u));
      v >>= le;
      used += le;
      int ds, dn;
      if (!decode<kTabBits>(sm.dist, v, ds, dn)) {
        br.skip(used);
        return br.bad_code();
      }
      if (ds > 29) return RMEM_PNG_ST_CODE;
      v >>= dn;
      const int de = ds < 4 ? 0 : (ds >> 1) - 1;
      const unsigned dist = (ds < 4 ? 1u + ds : 1u + ((2u + (ds & 1)) << de)) + ((unsigned)v & ((1u << de) - 1u));
      used += dn + de;                                  // <= 15 + 5 + 15 + 13 = 48 bits of the 64 peeked
      br.skip(used);
      if (br.overrun()) return RMEM_PNG_ST_INPUT;
      if (unsigned st = out.flush(lane)) return st;
      if (dist > out.pos) return RMEM_PNG_ST_RANGE;
      if (out.pos + len > out.N) return RMEM_PNG_ST_SIZE;
      copy_match(out, len, dist, lane);
    }
  }
  if (unsigned st = out.flush(lane)) return st;
  if (out.pos != out.N) return RMEM_PNG_ST_SIZE;        // the stream ends short of the frame
  br.bitpos = (br.bitpos + 7) & ~7ull;
  v = br.peek();
  br.skip(32);
  if (br.overrun()) return RMEM_PNG_ST_INPUT;
  const unsigned want = __builtin_bswap32((unsigned)v);
  uint64_t s1 = out.s1, s2 = out.s2;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  const unsigned a = (unsigned)((1 + s1) % kAdler), b = (unsigned)((out.N + s2) % kAdler);
  return (b << 16 | a) == want ? 0u : (unsigned)RMEM_PNG_ST_ADLER;
}

__device__ __forceinline__ bool desc_ok(const RmemPngDesc& d) {
  const bool depth_ok = d.colour_type == 3 ? (d.bit_depth == 1 || d.bit_depth == 2 || d.bit_depth == 4 || d.bit_depth == 8)
                                           : (d.colour_type == 0 && d.bit_depth == 8);
  return depth_ok && d.offset >= 0 && (d.offset & 7) == 0 && d.bytes >= 0;
}

__global__ __launch_bounds__(64) void k_pngd_inflate(const uint8_t* __restrict__ bits, const RmemPngDesc* __restrict__ descs, int H, int W,
                                                     size_t frame_ws, uint8_t* __restrict__ ws, int* __restrict__ status) {
  __shared__ Shared sm;
  const int f = blockIdx.x, lane = threadIdx.x;
  const RmemPngDesc d = descs[f];
  unsigned st = RMEM_PNG_ST_DESC;
  if (desc_ok(d)) {
    const uint32_t row_bytes = (uint32_t)(((uint64_t)W * d.bit_depth + 7) >> 3);
    BitReader br;
    br.init(bits + d.offset, (uint64_t)d.bytes);
    Sink out;
    out.dst = ws + (size_t)f * frame_ws;
    out.ring = sm.ring;
    out.N = (uint32_t)H * (row_bytes + 1u);             // <= 2^26 + H <= 2^27
    out.pos = 0;
    out.s1 = out.s2 = 0;
    out.pend = 0;
    out.npend = 0;
    st = inflate_stream(sm, br, out, lane);
  }
  if (lane == 0) status[f] = (int)st;
}

// One row by one 256-thread block: reconstruct (in place in the workspace unless the filter is None), unpack, table, store.
// `a` / `c` are thread 0's left and upper-left bytes carried over the 256-byte steps of an Average / Paeth row.
__device__ __forceinline__ void unfilter_row(uint8_t* __restrict__ src, size_t stride, int y, int ft, uint32_t row_bytes, int depth, int W,
                                             const uint8_t* s_lut, uint8_t* s_x, uint8_t* s_up, uint8_t* s_r, unsigned* s_wave,
                                             uint8_t* __restrict__ out_row) {
  const int t = threadIdx.x;
  uint8_t* const cur = src + (size_t)y * stride + 1;
  const uint8_t* const above = y > 0 ? cur - stride : nullptr;
  unsigned carry = 0;                                   // Sub: the reconstructed byte left of this step (every thread)
  unsigned a = 0, c = 0;                                // Average / Paeth: thread 0 only
  for (uint32_t i0 = 0; i0 < row_bytes; i0 += 256) {
    const uint32_t i = i0 + t;
    const bool active = i < row_bytes;
    const unsigned x = active ? cur[i] : 0u;
    const unsigned up = active && above && ft >= 2 ? above[i] : 0u;
    unsigned r = x;
    if (ft == 2) {
      r = (x + up) & 255u;
    } else if (ft == 1) {
      r = (block_excl_scan(x, s_wave, carry) + x) & 255u;
      carry &= 255u;
    } else if (ft >= 3) {
      s_x[t] = (uint8_t)x;
      s_up[t] = (uint8_t)up;
      __syncthreads();
      if (t == 0) {
        const int n = (int)std::min<uint32_t>(256u, row_bytes - i0);
        for (int j = 0; j < n; ++j) {
          const unsigned b = s_up[j];
          unsigned pred;
          if (ft == 3) {
            pred = (a + b) >> 1;
          } else {
            const int p = (int)a + (int)b - (int)c;
            const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
            pred = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
          }
          a = (s_x[j] + pred) & 255u;
          c = b;
          s_r[j] = (uint8_t)a;
        }
      }
      __syncthreads();
      r = s_r[t];
      __syncthreads();
    }
    if (!active) continue;
    if (ft != 0) cur[i] = (uint8_t)r;
    if (depth == 8) {
      out_row[i] = s_lut[r];
    } else {
      const int per = 8 / depth;
      const unsigned mask = (1u << depth) - 1u;
      for (int k = 0; k < per; ++k) {
        const uint64_t p = (uint64_t)i * per + k;
        if (p < (uint64_t)W) out_row[p] = s_lut[(r >> (8 - depth * (k + 1))) & mask];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_pngd_unfilter(const RmemPngDesc* __restrict__ descs, int H, int W, size_t frame_ws, uint8_t* __restrict__ ws,
                                                       const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int* __restrict__ status) {
  __shared__ uint8_t s_lut[256], s_x[256], s_up[256], s_r[256];
  __shared__ unsigned s_wave[4];
  const int f = blockIdx.y, slab = blockIdx.x, nslab = gridDim.x, t = threadIdx.x;
  s_lut[t] = lut ? lut[t] : (uint8_t)t;
  const int y0 = (int)((long)H * slab / nslab), y1 = (int)((long)H * (slab + 1) / nslab);
  uint8_t* const o = out + (size_t)f * H * W;
  uint8_t* const src = ws + (size_t)f * frame_ws;
  int st = status[f];                                   // slab 0 may already have added ST_FILTER: the same verdict as this block's
  int depth = 8;
  uint32_t row_bytes = 0;
  size_t stride = 0;
  int any = 0, bad = 0;
  if (st == 0) {
    depth = descs[f].bit_depth;                         // checked by k_pngd_inflate (ST_DESC otherwise)
    row_bytes = (uint32_t)(((uint64_t)W * depth + 7) >> 3);
    stride = (size_t)row_bytes + 1;
    for (int y = t; y < H; y += 256) {
      const int ft = src[(size_t)y * stride];
      any |= ft != 0;
      bad |= ft > 4;
    }
  }
  any = __syncthreads_or(any);
  bad = __syncthreads_or(bad);
  if (bad) {
    st = RMEM_PNG_ST_FILTER;
    if (slab == 0 && t == 0) status[f] = st;
  }
  if (st != 0) {                                        // nothing of an earlier call stays in `out`
    const size_t n = (size_t)(y1 - y0) * W;
    for (size_t i = t; i < n; i += 256) o[(size_t)y0 * W + i] = 0;
    return;
  }
  if (!any) {
    for (int y = y0; y < y1; ++y) unfilter_row(src, stride, y, 0, row_bytes, depth, W, s_lut, s_x, s_up, s_r, s_wave, o + (size_t)y * W);
  } else if (slab == 0) {
    for (int y = 0; y < H; ++y)
      unfilter_row(src, stride, y, src[(size_t)y * stride], row_bytes, depth, W, s_lut, s_x, s_up, s_r, s_wave, o + (size_t)y * W);
  }
}

inline size_t frame_workspace(int H, int W) { return align16((size_t)H * ((size_t)W + 1)); }

}  // namespace

extern "C" size_t rmem_png_decode_workspace_bytes(int frames, int H, int W) {
  if (!geometry_ok(frames, H, W)) return 0;
  return (size_t)frames * frame_workspace(H, W);        // the filtered bytes at depth 8, the widest accepted
}

extern "C" int rmem_png_decode_labels(const unsigned char* bits, const RmemPngDesc* descs, int frames, int H, int W, const unsigned char* lut,
                                      void* workspace, unsigned char* out, int* status, void* stream) {
  RMEM_REQUIRE(frames >= 1 && H >= 1 && W >= 1, "rmem_png_decode_labels: frames, H and W must be positive");
  RMEM_REQUIRE(frames <= 65535, "rmem_png_decode_labels: at most 65535 frames per call");
  RMEM_REQUIRE((long)H * W <= kMaxPixels, "rmem_png_decode_labels: frame too large (H * W must not exceed 2^26)");
  RMEM_REQUIRE(bits && descs && workspace && out && status, "rmem_png_decode_labels: null argument");
  RMEM_REQUIRE(((uintptr_t)bits & 7) == 0 && ((uintptr_t)workspace & 15) == 0,
               "rmem_png_decode_labels: bits must be 8-byte aligned and workspace 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t frame_ws = frame_workspace(H, W);
  hipLaunchKernelGGL(k_pngd_inflate, dim3(frames), dim3(64), 0, st, bits, descs, H, W, frame_ws, (uint8_t*)workspace, status);
  if (int rc = rmem_check_launch("rmem_png_decode_labels (inflate)")) return rc;
  const int slabs = std::max(1, std::min((H + 7) / 8, 1024 / frames));
  hipLaunchKernelGGL(k_pngd_unfilter, dim3(slabs, frames), dim3(256), 0, st, descs, H, W, frame_ws, (uint8_t*)workspace, lut, out, status);
  return rmem_check_launch("rmem_png_decode_labels (unfilter)");
}
