// Host side of the baseline JPEG decoder (include/rmem.h): marker parsing and the per-frame pack that the device decoder
// (jpeg.hip) reads.  Plain C++, no GPU: both run when a clip is loaded, not on the timed path.
#include "../../include/rmem.h"
#include <string.h>
#include <stdio.h>
#include <stdint.h>

extern "C" void rmem_set_error(const char* msg);

namespace {

const int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {
  int defined = 0;
  unsigned char counts[17] = {};
  unsigned char vals[256] = {};
};

struct Parsed {
  rmem_jpeg_info info;
  int comp_id[3], comp_td[3], comp_ta[3];
  HuffSpec huff[2][4];   // [0 = DC, 1 = AC][table id]
};

int fail(const char* why) {
  char b[256];
  snprintf(b, sizeof(b), "rmem_jpeg: %s", why);
  rmem_set_error(b);
  return -1;
}

inline int be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// Walks the markers up to the end of the single scan.  Fills everything rmem_jpeg_info reports plus the Huffman specs.
int parse_headers(const unsigned char* d, size_t n, Parsed* P) {
  memset(P, 0, sizeof(*P));
  rmem_jpeg_info& I = P->info;
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail("not a JPEG file (no SOI marker)");
  size_t pos = 2;
  int have_sof = 0, adobe = -1, jfif = 0;
  for (;;) {
    while (pos < n && d[pos] != 0xFF) pos++;             // tolerate junk between segments, as libjpeg does
    while (pos < n && d[pos] == 0xFF) pos++;             // fill bytes
    if (pos >= n) return fail("truncated file (no SOS marker)");
    const int m = d[pos++];
    if (m == 0xD9) return fail("no scan before EOI");
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // parameterless markers
    if (pos + 2 > n) return fail("truncated file (segment length)");
    const int len = be16(d + pos);
    if (len < 2 || pos + len > n) return fail("truncated file (segment)");
    const unsigned char* s = d + pos + 2;
    const int sl = len - 2;
    pos += len;
    if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) return fail("progressive JPEG (SOF2) unsupported");
    if (m >= 0xC9 && m <= 0xCF && m != 0xCC) return fail("arithmetic coding unsupported");
    if (m == 0xCC) return fail("arithmetic coding unsupported (DAC)");
    if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) return fail("lossless JPEG unsupported");
    if (m == 0xC5) return fail("hierarchical JPEG unsupported");
    if (m == 0xE0 && sl >= 5 && !memcmp(s, "JFIF", 5)) jfif = 1;
    if (m == 0xEE && sl >= 12 && !memcmp(s, "Adobe", 5)) adobe = s[11];
    if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (tq > 3) return fail("DQT table id > 3");
        const int need = 1 + 64 * (pq ? 2 : 1);
        if (pq > 1 || q + need > sl) return fail("bad DQT segment");
        for (int i = 0; i < 64; i++)
          I.quant[tq][kZigzag[i]] = pq ? (unsigned short)be16(s + q + 1 + 2 * i) : s[q + 1 + i];
        I.quant_mask |= 1 << tq;
        q += need;
      }
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        if (q + 17 > sl) return fail("bad DHT segment");
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return fail("bad DHT table class or id");
        HuffSpec& h = P->huff[tc][th];
        int total = 0;
        for (int l = 1; l <= 16; l++) total += (h.counts[l] = s[q + l]);
        if (total > 256 || q + 17 + total > sl) return fail("bad DHT segment");
        memcpy(h.vals, s + q + 17, total);
        h.defined = 1;
        q += 17 + total;
      }
    } else if (m == 0xDD) {
      if (sl < 2) return fail("bad DRI segment");
      I.restart_interval = be16(s);
    } else if (m == 0xC0 || m == 0xC1) {
      if (have_sof) return fail("more than one SOF");
      if (sl < 6) return fail("bad SOF segment");
      if (s[0] != 8) return fail("12-bit (or other non-8-bit) samples unsupported");
      I.height = be16(s + 1);
      I.width = be16(s + 3);
      I.components = s[5];
      if (I.height == 0) return fail("DNL-defined height unsupported");
      if (I.width == 0) return fail("zero width");
      if (I.components == 4) return fail("4 components (CMYK / YCCK) unsupported");
      if (I.components != 1 && I.components != 3) return fail("only 1 or 3 components are supported");
      if (sl < 6 + 3 * I.components) return fail("bad SOF segment");
      for (int c = 0; c < I.components; c++) {
        P->comp_id[c] = s[6 + 3 * c];
        I.h_samp[c] = s[7 + 3 * c] >> 4;
        I.v_samp[c] = s[7 + 3 * c] & 15;
        I.quant_id[c] = s[8 + 3 * c];
        if (I.h_samp[c] < 1 || I.h_samp[c] > 4 || I.v_samp[c] < 1 || I.v_samp[c] > 4 || I.quant_id[c] > 3)
          return fail("bad SOF component");
      }
      have_sof = 1;
    } else if (m == 0xDA) {
      if (!have_sof) return fail("SOS before SOF");
      const int ns = sl >= 1 ? s[0] : 0;
      if (sl < 1 + 2 * ns + 3) return fail("bad SOS segment");
      if (ns != I.components) return fail("multi-scan JPEG (a scan without every component) unsupported");
      for (int k = 0; k < ns; k++) {
        const int cs = s[1 + 2 * k];
        if (cs != P->comp_id[k]) return fail("multi-scan JPEG (scan components out of frame order) unsupported");
        P->comp_td[k] = s[2 + 2 * k] >> 4;
        P->comp_ta[k] = s[2 + 2 * k] & 15;
      }
      const unsigned char* t = s + 1 + 2 * ns;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return fail("progressive scan parameters in a sequential file");
      I.scan_begin = (long long)pos;
      break;
    }
  }
  // the entropy-coded segment ends at the first marker other than RSTn
  size_t e = (size_t)I.scan_begin;
  for (;;) {
    const void* f = memchr(d + e, 0xFF, n - e);
    if (!f) return fail("truncated file (entropy-coded segment has no end marker)");
    e = (const unsigned char*)f - d;
    if (e + 1 >= n) return fail("truncated file (entropy-coded segment has no end marker)");
    const int nx = d[e + 1];
    if (nx == 0x00 || (nx >= 0xD0 && nx <= 0xD7) || nx == 0xFF) { e += (nx == 0xFF) ? 1 : 2; continue; }
    break;
  }
  I.scan_end = (long long)e;
  {  // only EOI may follow the scan: walk what comes after it; a second SOS makes a multi-scan file
    size_t q = e;
    while (q + 3 < n) {
      while (q < n && d[q] == 0xFF) q++;
      if (q >= n) break;
      const int m = d[q++];
      if (m == 0xD9) break;
      if (m == 0xDA) return fail("multi-scan JPEG unsupported");
      if (m == 0xDC) return fail("DNL marker unsupported");
      if (q + 2 > n) break;
      q += be16(d + q);
      if (q < n && d[q] != 0xFF) break;                 // not a marker segment: trailing data
    }
  }
  // colour model: libjpeg treats an Adobe transform 0 or R/G/B component ids without JFIF as RGB (no YCbCr conversion)
  if (I.components == 3 && (adobe == 0 || (!jfif && adobe < 0 && P->comp_id[0] == 'R' && P->comp_id[1] == 'G' &&
                                           P->comp_id[2] == 'B')))
    return fail("RGB JPEG (no YCbCr transform) unsupported");
  if (I.components == 3) {
    const int h0 = I.h_samp[0], v0 = I.v_samp[0];
    const int ok = I.h_samp[1] == 1 && I.v_samp[1] == 1 && I.h_samp[2] == 1 && I.v_samp[2] == 1 &&
                   ((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2));
    if (!ok) return fail("sampling unsupported (supported: 4:4:4, 4:2:2 h2v1, 4:2:0 h2v2, grayscale)");
  }
  for (int c = 0; c < I.components; c++) {
    if (!(I.quant_mask >> I.quant_id[c] & 1)) return fail("missing quantisation table");
    if (P->comp_td[c] > 3 || P->comp_ta[c] > 3 || !P->huff[0][P->comp_td[c]].defined || !P->huff[1][P->comp_ta[c]].defined)
      return fail("missing Huffman table");
  }
  const int hmax = I.components == 1 ? 1 : I.h_samp[0], vmax = I.components == 1 ? 1 : I.v_samp[0];
  const long long mcus = (long long)((I.width + 8 * hmax - 1) / (8 * hmax)) * ((I.height + 8 * vmax - 1) / (8 * vmax));
  const long long units = I.restart_interval ? (mcus + I.restart_interval - 1) / I.restart_interval : 1;
  I.packed_bound = 16 + ((units + 1) * 8 + 15) / 16 * 16 + (I.scan_end - I.scan_begin) + 48;
  return 0;
}

int build_huff(const HuffSpec& s, int is_dc, rmem_jpeg_huff* h) {
  memset(h, 0, sizeof(*h));
  int code = 0, k = 0;
  for (int l = 1; l <= 16; l++) {
    h->maxcode[l] = -1;
    if (s.counts[l]) {
      h->valoff[l] = k - code;
      for (int i = 0; i < s.counts[l]; i++, k++, code++) {
        const int sym = s.vals[k];
        if (is_dc && sym > 11) return fail("DC Huffman symbol > 11");
        if (l <= 9)
          for (int j = code << (9 - l); j < (code + 1) << (9 - l); j++) h->lut[j] = (unsigned short)((l << 8) | sym);
      }
      h->maxcode[l] = code - 1;
      if (code > (1 << l)) return fail("bad Huffman table (code space overflow)");
    }
    code <<= 1;
  }
  memcpy(h->vals, s.vals, 256);
  return 0;
}

}  // namespace

extern "C" int rmem_jpeg_parse(const unsigned char* data, size_t n, rmem_jpeg_info* out) {
  if (!out) return fail("null output");
  Parsed P;
  const int rc = parse_headers(data, n, &P);
  if (rc) return rc;
  *out = P.info;
  return 0;
}

extern "C" int rmem_jpeg_pack(const unsigned char* data, size_t n, unsigned char* buf, size_t cap, size_t* used,
                              rmem_jpeg_desc* desc) {
  if (!buf || !used || !desc) return fail("rmem_jpeg_pack: null argument");
  Parsed P;
  if (parse_headers(data, n, &P)) return -1;
  const rmem_jpeg_info& I = P.info;
  rmem_jpeg_desc D;
  memset(&D, 0, sizeof(D));
  D.width = I.width;
  D.height = I.height;
  D.ncomp = I.components;
  const int gray = I.components == 1;
  D.hmax = gray ? 1 : I.h_samp[0];
  D.vmax = gray ? 1 : I.v_samp[0];
  D.mcus_x = (I.width + 8 * D.hmax - 1) / (8 * D.hmax);
  D.mcus_y = (I.height + 8 * D.vmax - 1) / (8 * D.vmax);
  int b = 0, blk0 = 0;
  for (int c = 0; c < D.ncomp; c++) {
    const int h = gray ? 1 : I.h_samp[c], v = gray ? 1 : I.v_samp[c];
    D.comp_h[c] = h;
    D.comp_v[c] = v;
    D.comp_bw[c] = D.mcus_x * h;
    D.comp_bh[c] = D.mcus_y * v;
    D.comp_block0[c] = blk0;
    blk0 += D.comp_bw[c] * D.comp_bh[c];
    D.comp_dw[c] = (I.width * h + D.hmax - 1) / D.hmax;
    D.comp_dh[c] = (I.height * v + D.vmax - 1) / D.vmax;
    for (int i = 0; i < h * v; i++, b++) {
      D.mcu_comp[b] = c;
      D.mcu_sub[b] = i;
    }
    for (int i = 0; i < 64; i++) D.quant[c][i] = I.quant[I.quant_id[c]][i];
    if (build_huff(P.huff[0][P.comp_td[c]], 1, &D.dc[c]) || build_huff(P.huff[1][P.comp_ta[c]], 0, &D.ac[c])) return -1;
  }
  D.bpm = b;
  D.total_blocks = blk0;
  const long long mcus = (long long)D.mcus_x * D.mcus_y;
  D.restart_mcus = I.restart_interval;
  const long long units = I.restart_interval ? (mcus + I.restart_interval - 1) / I.restart_interval : 1;
  if (mcus * D.bpm > (1LL << 30) || units > (1 << 24)) return fail("image too large");
  D.nunits = (int)units;
  const size_t start = (*used + 15) & ~(size_t)15;
  const size_t table = ((size_t)(units + 1) * 8 + 15) & ~(size_t)15;
  const size_t scan = (size_t)(I.scan_end - I.scan_begin);
  if (start + table + scan + 32 > cap) return fail("rmem_jpeg_pack: buffer too small (see rmem_jpeg_info.packed_bound)");
  D.offset = (long long)start;
  D.data_off = (int)table;
  uint32_t* tab = (uint32_t*)(buf + start);
  unsigned char* out = buf + start + table;
  // strip FF 00 stuffing and RSTn markers: memchr for the next FF, memcpy the run before it
  const unsigned char* p = data + I.scan_begin;
  const unsigned char* const e = data + I.scan_end;
  size_t o = 0;
  long long u = 0;
  uint32_t sub = 0;
  long long ubegin = 0;
  auto close_unit = [&](size_t end_byte) {
    const long long bits = (long long)(end_byte - ubegin) * 8;
    tab[2 * u] = (uint32_t)(ubegin * 8);
    tab[2 * u + 1] = sub;
    sub += bits > 0 ? (uint32_t)((bits + RMEM_JPEG_SUBSEQ_BITS - 1) / RMEM_JPEG_SUBSEQ_BITS) : 1;
    u++;
  };
  while (p < e) {
    const unsigned char* f = (const unsigned char*)memchr(p, 0xFF, e - p);
    const unsigned char* run_end = f ? f : e;
    memcpy(out + o, p, run_end - p);
    o += run_end - p;
    if (!f) break;
    int nx = f + 1 < e ? f[1] : 0;
    p = f + 1;
    while (nx == 0xFF && p + 1 < e) nx = *++p;   // FF fill bytes before a marker
    if (nx == 0x00) {
      out[o++] = 0xFF;
      p++;
    } else if (nx >= 0xD0 && nx <= 0xD7) {
      if (u + 1 >= units) return fail("more restart markers than restart intervals");
      close_unit(o);
      ubegin = (long long)o;
      p++;
    } else {
      return fail("unexpected marker inside the entropy-coded segment");
    }
  }
  if (u + 1 != units) return fail("fewer restart markers than restart intervals");
  close_unit(o);
  tab[2 * u] = (uint32_t)(o * 8);
  tab[2 * u + 1] = sub;
  if (o * 8 >= (1ULL << 31)) return fail("entropy-coded segment too large");
  memset(out + o, 0, 32);
  D.nsub = (int)sub;
  D.data_bits = (int)(o * 8);
  D.bytes = (long long)(table + ((o + 32 + 15) & ~(size_t)15));
  *used = start + (size_t)D.bytes;
  *desc = D;
  return 0;
}
