"""A plain-Python restatement of what rmem_png_decode_labels reads (include/rmem.h): RFC 1950 / 1951 inflate bit by bit, the five
PNG row filters, sample unpacking -- the tests' reference for the device decoder -- and a PNG builder with the case table both test
tiers run.  Independent of rmem_ocu_amd.

    inflate(stream)        zlib stream -> (bytes, Stats): what zlib.decompress gives, plus what the stream contains
    deflate_fixed(tokens)  a hand-chosen token list -> zlib stream with the fixed codes (streams zlib's own compressor never writes)
    build_png(...)         label map -> PNG file with chosen bit depth, colour type, per-row filters, DEFLATE flavour, IDAT split
    decode_png(data)       PNG file -> label map, through inflate / unfilter / unpack above
    cases()                name -> Case(png, label, claims); assert_cases_exercise_what_they_claim() checks the claims on the CPU
    corrupt_cases()        name -> (png, the one status bit the decoder must report)
"""
import functools
import io
import struct
import zlib
from collections import namedtuple

import numpy as np

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ST_INPUT, ST_SIZE, ST_RANGE, ST_CODE, ST_HEADER, ST_ADLER, ST_FILTER, ST_DESC = 1, 2, 4, 8, 16, 32, 64, 128
SIGNATURE = b'\x89PNG\r\n\x1a\n'


class Stats:
    def __init__(self):
        self.block_types = set()
        self.max_litlen_bits = 0        # the longest literal/length code USED
        self.max_dist_bits = 0
        self.max_distance = 0
        self.tokens = 0
        self.min_dist_len_ratio = None  # smallest distance / length over the matches: below 1 = an overlapping copy
        self.matches = []               # (length, distance)
        self.stored_lens = []
        self.dist_code_lengths = []     # per dynamic block: the non-zero distance code lengths
        self.litlen_bits_used = set()


class _Bits:
    def __init__(self, data):
        self.d, self.pos = bytes(data), 0

    def bit(self):
        if self.pos >> 3 >= len(self.d):
            raise ValueError('inflate: the stream ends too early')
        b = self.d[self.pos >> 3] >> (self.pos & 7) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v


class _Code:
    """canonical Huffman code from a list of lengths; decode walks it one bit at a time (RFC 1951 3.2.2)"""

    def __init__(self, lengths):
        self.count = [0] * 16
        for l in lengths:
            self.count[l] += 1
        self.count[0] = 0
        left = 1
        for l in range(1, 16):
            left = left * 2 - self.count[l]
            if left < 0:
                raise ValueError('inflate: over-subscribed code')
        self.incomplete = left > 0
        self.symbols = [s for l in range(1, 16) for s, sl in enumerate(lengths) if sl == l]

    def decode(self, br):
        code = first = index = 0
        for l in range(1, 16):
            code |= br.bit()
            c = self.count[l]
            if code - c < first:
                return self.symbols[index + code - first], l
            index += c
            first = (first + c) << 1
            code <<= 1
        raise ValueError('inflate: invalid code')


def _fixed_codes():
    return _Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _Code([5] * 32)


def inflate(stream):
    """zlib stream -> (inflated bytes, Stats); ValueError on anything zlib would refuse"""
    stream = bytes(stream)
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 32:
        raise ValueError('inflate: bad zlib header')
    br, out, st = _Bits(stream[2:]), bytearray(), Stats()
    last = 0
    while not last:
        last, btype = br.bit(), br.bits(2)
        st.block_types.add(btype)
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.bits(16), br.bits(16)
            if n != (~nn & 0xFFFF):
                raise ValueError('inflate: stored LEN / NLEN mismatch')
            at = br.pos >> 3
            if at + n > len(br.d):
                raise ValueError('inflate: the stream ends too early')
            out += br.d[at:at + n]
            br.pos += 8 * n
            st.stored_lens.append(n)
            continue
        if btype == 3:
            raise ValueError('inflate: block type 3')
        if btype == 1:
            lit, dist = _fixed_codes()
        else:
            hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
            if hlit > 286 or hdist > 30:
                raise ValueError('inflate: too many symbols')
            cl = [0] * 19
            for i in range(hclen):
                cl[CL_ORDER[i]] = br.bits(3)
            clc = _Code(cl)
            if clc.incomplete:
                raise ValueError('inflate: incomplete code-length code')
            lens = []
            while len(lens) < hlit + hdist:                 # ONE sequence: a repeat may run across the literal / distance boundary
                s, _ = clc.decode(br)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    if not lens:
                        raise ValueError('inflate: repeat with no previous length')
                    lens += [lens[-1]] * (3 + br.bits(2))
                elif s == 17:
                    lens += [0] * (3 + br.bits(3))
                else:
                    lens += [0] * (11 + br.bits(7))
            if len(lens) > hlit + hdist:
                raise ValueError('inflate: lengths overrun')
            if lens[256] == 0:
                raise ValueError('inflate: no end-of-block code')
            lit, dist = _Code(lens[:hlit]), _Code(lens[hlit:])
            used = [l for l in lens[hlit:] if l]
            st.dist_code_lengths.append(used)
            if lit.incomplete and max(lens[:hlit]) != 1 or dist.incomplete and used and max(used) != 1:
                raise ValueError('inflate: incomplete code')
        while True:
            s, l = lit.decode(br)
            st.max_litlen_bits = max(st.max_litlen_bits, l)
            st.litlen_bits_used.add(l)
            st.tokens += 1
            if s < 256:
                out.append(s)
            elif s == 256:
                st.tokens -= 1
                break
            else:
                if s > 285:
                    raise ValueError('inflate: invalid length symbol')
                n = LENGTH_BASE[s - 257] + br.bits(LENGTH_EXTRA[s - 257])
                ds, dl = dist.decode(br)
                if ds > 29:
                    raise ValueError('inflate: invalid distance symbol')
                d = DIST_BASE[ds] + br.bits(DIST_EXTRA[ds])
                if d > len(out):
                    raise ValueError('inflate: distance too far back')
                st.max_dist_bits = max(st.max_dist_bits, dl)
                st.max_distance = max(st.max_distance, d)
                st.min_dist_len_ratio = d / n if st.min_dist_len_ratio is None else min(st.min_dist_len_ratio, d / n)
                st.matches.append((n, d))
                for _ in range(n):
                    out.append(out[-d])
    br.pos = (br.pos + 7) & ~7
    at = br.pos >> 3
    if at + 4 > len(br.d):
        raise ValueError('inflate: the stream ends too early')
    if struct.unpack('>I', br.d[at:at + 4])[0] != zlib.adler32(bytes(out)) & 0xFFFFFFFF:
        raise ValueError('inflate: Adler-32 mismatch')
    return bytes(out), st


# ------------------------------------------------------------------------------------------------------------- writing streams

class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        """n bits of value, least significant first"""
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huffman(self, code, n):
        """a Huffman code: most significant bit first"""
        for i in range(n - 1, -1, -1):
            self.bits(code >> i & 1, 1)

    def finish(self):
        if self.n:
            self.buf.append(self.acc & 255)
            self.acc = self.n = 0
        return bytes(self.buf)


def fixed_code(sym):
    """RFC 1951 3.2.6: (code, bits) of literal / length symbol sym"""
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def _index(base, v):
    return max(i for i, b in enumerate(base) if b <= v)


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == 'lit':
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def deflate_fixed(tokens, adler=None):
    """zlib stream (78 01, one final fixed-Huffman block, Adler-32) of ('lit', v) / ('match', length, distance) tokens.  adler: the
    trailer to write instead of the Adler-32 of the tokens' expansion (for streams whose tokens do not expand)."""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for t in tokens:
        if t[0] == 'lit':
            w.huffman(*fixed_code(t[1]))
        else:
            _, n, d = t
            li = 28 if n == 258 else _index(LENGTH_BASE[:28], n)
            w.huffman(*fixed_code(257 + li))
            w.bits(n - LENGTH_BASE[li], LENGTH_EXTRA[li])
            di = _index(DIST_BASE, d)
            w.huffman(di, 5)
            w.bits(d - DIST_BASE[di], DIST_EXTRA[di])
    w.huffman(*fixed_code(256))
    if adler is None:
        adler = zlib.adler32(expand(tokens)) & 0xFFFFFFFF
    return b'\x78\x01' + w.finish() + struct.pack('>I', adler)


def huffman_lengths(freqs):
    """{symbol: code length} of a Huffman code for {symbol: frequency > 0} (at least two symbols)"""
    import heapq
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freqs.items()))]
    heapq.heapify(heap)
    lens = dict.fromkeys(freqs, 0)
    k = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for sym in a[2] + b[2]:
            lens[sym] += 1
        heapq.heappush(heap, (a[0] + b[0], k, a[2] + b[2]))
        k += 1
    assert max(lens.values()) <= 15
    return lens


def canonical_codes(lens):
    """{symbol: (code, length)} for {symbol: length}"""
    code, out = 0, {}
    for l in range(1, 16):
        for sym in sorted(s for s, sl in lens.items() if sl == l):
            out[sym] = (code, l)
            code += 1
        code <<= 1
    return out


def deflate_dynamic(tokens, lit_lens=None, dist_lens=None, hlit=None):
    """zlib stream of ONE dynamic block of the tokens.  lit_lens / dist_lens: {symbol: code length}, by default Huffman codes of
    the tokens' own frequencies; dist_lens may be {} (HDIST = 1, that one length 0: no distance code at all) or a single code of
    length 1 (the incomplete code zlib's decoder allows) -- two headers zlib's compressor never writes.  The code lengths go out
    as one sequence over the literal/length and the distance lengths, runs coded with 16 / 17 / 18 wherever they fit, also across
    the boundary between the two."""
    syms, dsyms = [], []
    for t in tokens:
        if t[0] == 'lit':
            syms.append((t[1],))
        else:
            li = 28 if t[1] == 258 else _index(LENGTH_BASE[:28], t[1])
            di = _index(DIST_BASE, t[2])
            syms.append((257 + li, t[1] - LENGTH_BASE[li], LENGTH_EXTRA[li], di, t[2] - DIST_BASE[di], DIST_EXTRA[di]))
            dsyms.append(di)
    if lit_lens is None:
        freq = {256: 1}
        for t in syms:
            freq[t[0]] = freq.get(t[0], 0) + 1
        lit_lens = huffman_lengths(freq)
    if dist_lens is None:
        freq = {}
        for d in dsyms:
            freq[d] = freq.get(d, 0) + 1
        dist_lens = {} if not freq else {next(iter(freq)): 1} if len(freq) == 1 else huffman_lengths(freq)
    hlit = max(257, max(lit_lens) + 1) if hlit is None else hlit
    hdist = max(1, max(dist_lens, default=0) + 1)
    seq = [lit_lens.get(i, 0) for i in range(hlit)] + [dist_lens.get(i, 0) for i in range(hdist)]
    cl_codes = canonical_codes({**{i: 5 for i in range(16)}, 16: 3, 17: 3, 18: 2})       # a complete code-length code
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(hlit - 257, 5), w.bits(hdist - 1, 5), w.bits(15, 4)
    for sym in CL_ORDER:
        w.bits(cl_codes[sym][1], 3)
    i = 0
    while i < len(seq):
        run = 1
        while i + run < len(seq) and seq[i + run] == seq[i]:
            run += 1
        if seq[i] == 0 and run >= 3:
            n = min(run, 138)
            w.huffman(*cl_codes[18 if n >= 11 else 17])
            w.bits(n - (11 if n >= 11 else 3), 7 if n >= 11 else 3)
            i += n
        elif i > 0 and seq[i] == seq[i - 1] and run >= 3:
            n = min(run, 6)
            w.huffman(*cl_codes[16])
            w.bits(n - 3, 2)
            i += n
        else:
            w.huffman(*cl_codes[seq[i]])
            i += 1
    lit, dist = canonical_codes(lit_lens), canonical_codes(dist_lens)
    for t in syms:
        w.huffman(*lit[t[0]])
        if len(t) > 1:
            w.bits(t[1], t[2])
            w.huffman(*dist[t[3]])
            w.bits(t[4], t[5])
    w.huffman(*lit[256])
    return b'\x78\x01' + w.finish() + struct.pack('>I', zlib.adler32(expand(tokens)) & 0xFFFFFFFF)


def rle_tokens(data):
    """a literal, then distance-1 matches of up to 258, for every run of at least 4 equal bytes; literals otherwise"""
    data, toks, i = bytes(data), [], 0
    while i < len(data):
        run = 1
        while i + run < len(data) and data[i + run] == data[i]:
            run += 1
        toks.append(('lit', data[i]))
        rem = run - 1
        while rem >= 3:
            n = min(rem, 258)
            toks.append(('match', n, 1))
            rem -= n
        toks += [('lit', data[i])] * rem
        i += run
    return toks


def tokens_with_matches(data, matches):
    """literals for every byte of data except the given (position, length, distance) matches, which must hold in data"""
    data, toks, at = bytes(data), [], 0
    for pos, n, d in sorted(matches):
        assert pos >= at and d <= pos and all(data[pos + i] == data[pos + i - d] for i in range(n)), (pos, n, d)
        toks += [('lit', v) for v in data[at:pos]] + [('match', n, d)]
        at = pos + n
    return toks + [('lit', v) for v in data[at:]]


def stored_stream(data, sizes):
    """zlib stream of stored blocks of the given sizes (they must add up to len(data); 0 is allowed)"""
    assert sum(sizes) == len(data)
    out, at = bytearray(b'\x78\x01'), 0
    for k, n in enumerate(sizes):
        out += bytes([1 if k == len(sizes) - 1 else 0]) + struct.pack('<HH', n, ~n & 0xFFFF) + data[at:at + n]
        at += n
    return bytes(out) + struct.pack('>I', zlib.adler32(bytes(data)) & 0xFFFFFFFF)


def compress(data, how):
    data = bytes(data)
    if callable(how):
        return how(data)
    if not isinstance(how, str):
        return deflate_fixed(how)
    if how == 'stored':
        return zlib.compress(data, 0)
    if how == 'stored_edges':           # LEN = 0, then the largest stored block, then the rest
        n = min(len(data), 65535)
        return stored_stream(data, [0, n, len(data) - n])
    if how == 'multi':                  # a full flush every 997 bytes: empty stored blocks between blocks of whatever type zlib picks
        c = zlib.compressobj(6)
        parts = [c.compress(data[i:i + 997]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(data), 997)]
        return b''.join(parts) + c.flush(zlib.Z_FINISH)
    strategy = {'fixed': zlib.Z_FIXED, 'dynamic': zlib.Z_DEFAULT_STRATEGY, 'huffman_only': zlib.Z_HUFFMAN_ONLY, 'rle': zlib.Z_RLE}[how]
    c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(data) + c.flush()


# ------------------------------------------------------------------------------------------------------------- filters, samples

def pack_rows(lab, depth, pad_ones=True):
    """uint8 [H, ceil(W * depth / 8)]: samples most significant bits first; the padding bits at the end of a row are ones"""
    lab = np.asarray(lab, dtype=np.uint8)
    H, W = lab.shape
    if depth == 8:
        return lab.copy()
    per = 8 // depth
    rb = -(-W // per)
    padded = np.full((H, rb * per), (1 << depth) - 1 if pad_ones else 0, dtype=np.uint8)
    assert lab.max() < 1 << depth
    padded[:, :W] = lab
    out = np.zeros((H, rb), dtype=np.uint8)
    for k in range(per):
        out |= padded[:, k::per] << (8 - depth * (k + 1))
    return out


def unpack_rows(rows, depth, W):
    rows = np.asarray(rows, dtype=np.uint8)
    if depth == 8:
        return rows[:, :W].copy()
    per = 8 // depth
    out = np.zeros((rows.shape[0], rows.shape[1] * per), dtype=np.uint8)
    for k in range(per):
        out[:, k::per] = rows >> (8 - depth * (k + 1)) & ((1 << depth) - 1)
    return out[:, :W]


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(rows, filters):
    """uint8 [H, 1 + rb]: per row the filter type, then the filtered bytes (filter unit: one byte)"""
    rows = np.asarray(rows, dtype=np.uint8).astype(np.int64)
    H, rb = rows.shape
    out = np.zeros((H, rb + 1), dtype=np.uint8)
    for y, ft in enumerate(filters):
        cur = rows[y]
        up = rows[y - 1] if y else np.zeros(rb, dtype=np.int64)
        left = np.concatenate(([0], cur[:-1]))
        ul = np.concatenate(([0], up[:-1]))
        pred = [np.zeros(rb, dtype=np.int64), left, up, (left + up) >> 1, None][ft]
        if ft == 4:
            pa, pb, pc = abs(up - ul), abs(left - ul), abs(left + up - 2 * ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out


def unfilter_rows(filt):
    """the inverse, byte by byte"""
    filt = np.asarray(filt, dtype=np.uint8)
    H, rb = filt.shape[0], filt.shape[1] - 1
    rows = np.zeros((H, rb), dtype=np.int64)
    for y in range(H):
        ft = int(filt[y, 0])
        if ft > 4:
            raise ValueError('filter type above 4')
        x = filt[y, 1:].astype(np.int64)
        up = rows[y - 1] if y else np.zeros(rb, dtype=np.int64)
        if ft == 0:
            rows[y] = x
        elif ft == 2:
            rows[y] = (x + up) & 255
        elif ft == 1:
            rows[y] = np.cumsum(x) & 255
        else:
            a = c = 0
            for i in range(rb):
                b = int(up[i])
                a = (int(x[i]) + ((a + b) >> 1 if ft == 3 else _paeth(a, b, c))) & 255
                c = b
                rows[y, i] = a
    return rows.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- files

def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_around(stream, H, W, depth=8, colour_type=3, idat_split=None, interlace=0, extra=b''):
    """a PNG file around one zlib stream, cut into IDAT chunks of idat_split bytes; an ancillary tEXt chunk comes first"""
    n = len(stream) if not idat_split else idat_split
    idats = b''.join(chunk(b'IDAT', stream[i:i + n]) for i in range(0, max(len(stream), 1), n))
    plte = chunk(b'PLTE', bytes(range(256)) * 3) if colour_type == 3 else b''
    return (SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, colour_type, 0, 0, interlace)) + chunk(b'tEXt', b'k\x00v')
            + plte + extra + idats + chunk(b'IEND', b''))


def filtered_bytes(lab, depth=8, filters=None):
    lab = np.asarray(lab, dtype=np.uint8)
    return filter_rows(pack_rows(lab, depth), [0] * lab.shape[0] if filters is None else filters).tobytes()


def build_png(lab, depth=8, colour_type=3, filters=None, compress_how='dynamic', idat_split=None):
    lab = np.asarray(lab, dtype=np.uint8)
    return png_around(compress(filtered_bytes(lab, depth, filters), compress_how), lab.shape[0], lab.shape[1], depth, colour_type, idat_split)


def split_png(data):
    """(IHDR fields, zlib stream) of a PNG file; checks every CRC"""
    assert data[:8] == SIGNATURE
    at, ihdr, stream = 8, None, b''
    while at < len(data):
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0]
        if kind == b'IHDR':
            ihdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            stream += body
        at += 12 + n
    return ihdr, stream


def decode_png(data):
    """PNG file -> uint8 [H, W] samples (palette indices or grey values) through this file's inflate, unfilter and unpack"""
    (W, H, depth, ctype, _, _, interlace), stream = split_png(data)
    assert interlace == 0 and ctype in (0, 3)
    raw, _ = inflate(stream)
    rb = (W * depth + 7) // 8
    assert len(raw) == H * (rb + 1)
    return unpack_rows(unfilter_rows(np.frombuffer(raw, dtype=np.uint8).reshape(H, rb + 1)), depth, W)


# ------------------------------------------------------------------------------------------------------------- the case table

Case = namedtuple('Case', 'png label claims lut')      # claims: what assert_cases_exercise_what_they_claim checks; lut: or None


def _pillow(lab, **kw):
    from PIL import Image
    im = Image.fromarray(np.asarray(lab, dtype=np.uint8), mode='P')
    im.putpalette(list(range(256)) * 3)
    buf = io.BytesIO()
    im.save(buf, format='PNG', **kw)
    return buf.getvalue()


def noise(H, W, top, seed):
    return np.random.RandomState(seed).randint(0, top, (H, W)).astype(np.uint8)


def long_code_map():
    """64 x 200 labels 0 .. 14, value v about half as frequent as v - 1 but each present at least 40 times"""
    rs = np.random.RandomState(21)
    lab = np.minimum(rs.geometric(0.5, (64, 200)) - 1, 14).astype(np.uint8)
    flat = lab.reshape(-1)
    for v in range(15):
        flat[rs.randint(0, flat.size, 40)] = v
    return lab


def periodic_row(d, W=326):
    """1 x W: the first d pixels distinct, then period d for 258 pixels (a match of length 258 at distance d), then a tail"""
    row = np.zeros(W, dtype=np.uint8)
    row[:d] = np.arange(1, d + 1)
    for i in range(d, d + 258):
        row[i] = row[i - d]
    row[d + 258:] = np.arange(200, 200 + W - d - 258)
    return row[None]


def far_map():
    """200 x 200 noise whose bytes 32975 .. 33075 of the filtered stream repeat the ones 32768 before"""
    lab = noise(200, 200, 16, 31)
    filt = np.frombuffer(filtered_bytes(lab), dtype=np.uint8).copy()
    filt[32975:33075] = filt[32975 - 32768:33075 - 32768]
    assert (32975 - 1) // 201 == (33075 - 1) // 201         # inside one row, no filter byte touched
    return filt.reshape(200, 201)[:, 1:].copy()


@functools.lru_cache(maxsize=None)
def cases():
    from boundary_ref import blobs
    import png_ref
    out = {}

    def add(name, lab, claims=(), lut=None, png=None, **kw):
        lab = np.asarray(lab, dtype=np.uint8)
        out[name] = Case(build_png(lab, **kw) if png is None else png, lab, dict(claims), lut)

    # shape edges
    add('edge_1x1', [[3]])
    add('edge_1x70', noise(1, 70, 5, 1))
    add('edge_70x1', noise(70, 1, 5, 2))
    add('edge_5x7', noise(5, 7, 256, 3))
    for w in (63, 64, 65, 129):
        add(f'edge_5x{w}', noise(5, w, 7, w), filters=[0, 1, 2, 3, 4])
    add('blobs10_97x131', blobs(97, 131, 11, seed=5), {'block_types': {2}})
    # bit depths below 8, the padding bits of every row set
    for w in (1, 7, 8, 9, 13):
        for depth in (1, 2, 4):
            add(f'depth{depth}_3x{w}', noise(3, w, 1 << depth, 10 * w + depth), {'depth': depth, 'filters': {0, 1, 4}}, depth=depth,
                filters=[0, 1, 4])
    # 8-bit grey, 0 / 255, read through the table 255 -> 1
    lut = np.arange(256, dtype=np.uint8)
    lut[255] = 1
    add('grey_40x50', (blobs(40, 50, 2, seed=6) > 0) * np.uint8(255), {'colour_type': 0}, lut=lut, colour_type=0)
    # the five filters on uniform noise
    nz = noise(64, 200, 256, 7)
    for ft in range(5):
        add(f'filter{ft}_64x200', nz, {'filters': {ft}}, filters=[ft] * 64, compress_how='fixed' if ft == 0 else 'dynamic')
    add('filtermix_64x200', nz, {'filters': {0, 1, 2, 3, 4}}, filters=np.random.RandomState(8).randint(0, 5, 64).tolist())
    # DEFLATE flavours on one blob map
    bl = blobs(64, 200, 6, seed=9)
    add('stored_64x200', bl, {'block_types': {0}}, compress_how='stored')
    add('fixed_64x200', bl, {'block_types': {1}}, compress_how='fixed')
    add('huffman_only_64x200', bl, {'block_types': {2}, 'no_matches': True}, compress_how='huffman_only')
    add('rle_64x200', bl, {'block_types': {2}, 'max_distance': 1}, compress_how='rle')
    # zlib's compressor always sends two distance codes; the two headers it never writes: no distance code at all (the code lengths'
    # run of zeros crosses from the literal/length into the distance lengths), and a single one-bit distance code (incomplete)
    add('no_dist_code_64x200', bl, {'block_types': {2}, 'no_dist_code': True},
        compress_how=lambda d: deflate_dynamic([('lit', v) for v in d], dist_lens={}, hlit=261))
    add('single_dist_code_64x200', bl, {'block_types': {2}, 'single_dist_code': True, 'max_distance': 1},
        compress_how=lambda d: deflate_dynamic(rle_tokens(d)))
    add('multi_64x200', nz, {'block_types_include': {0}, 'stored_len': 0, 'blocks_min': 13}, compress_how='multi', idat_split=4096)
    add('idat7_64x200', bl, {}, compress_how='dynamic', idat_split=7)
    add('idat1_5x7', noise(5, 7, 256, 3), {}, idat_split=1)
    # stored blocks of LEN = 0 and 65535
    add('stored_edges_256x256', noise(256, 256, 4, 12), {'block_types': {0}, 'stored_len': 65535, 'stored_len2': 0}, compress_how='stored_edges')
    # overlapping copies: a match of 258 at distances around the wave width
    for d in (1, 2, 3, 63, 64, 65):
        lab = periodic_row(d)
        toks = tokens_with_matches(filtered_bytes(lab), [(1 + d, 258, d)])
        add(f'overlap_d{d}_1x326', lab, {'block_types': {1}, 'match': (258, d)}, compress_how=toks)
    # the largest distance
    lab = far_map()
    add('far_200x200', lab, {'match': (100, 32768), 'max_distance': 32768},
        compress_how=tokens_with_matches(filtered_bytes(lab), [(32975, 100, 32768)]))
    # code lengths 1 .. 15: literals 0 .. 14 of lengths 1 .. 15 and the end-of-block code of length 15, a complete code
    lengths = {**{v: v + 1 for v in range(15)}, 256: 15}
    add('long_codes_64x200', long_code_map(), {'block_types': {2}, 'max_litlen_bits': 15, 'litlen_bits_used': set(range(1, 16))},
        compress_how=lambda d: deflate_dynamic([('lit', v) for v in d], lit_lens=lengths, dist_lens={}))
    # Pillow's own files
    pl = blobs(97, 131, 11, seed=13)
    add('pillow_97x131', pl, {'filters': {0}}, png=_pillow(pl))
    add('pillow_opt_97x131', pl, {'filters': {0}}, png=_pillow(pl, optimize=True))
    add('pillow_bits4_97x131', pl, {'depth': 4}, png=_pillow(pl, bits=4))
    # the project's own writer
    add('roundtrip_97x131', pl, {'block_types': {1}, 'filters': {2}, 'max_distance': 1}, png=png_ref.wrap(png_ref.zlib_stream(pl), 97, 131))
    return out


def case_names():
    return list(cases())


def assert_cases_exercise_what_they_claim():
    """a condition on the inputs, checked on the CPU: every case really contains what its name says"""
    for name, c in cases().items():
        (W, H, depth, ctype, _, _, _), stream = split_png(c.png)
        raw, st = inflate(stream)
        assert (H, W) == c.label.shape, name
        rb = (W * depth + 7) // 8
        fts = set(np.frombuffer(raw, dtype=np.uint8).reshape(H, rb + 1)[:, 0].tolist())
        for key, want in c.claims.items():
            got = {'block_types': st.block_types, 'depth': depth, 'colour_type': ctype, 'filters': fts, 'max_litlen_bits': st.max_litlen_bits,
                   'max_distance': st.max_distance, 'litlen_bits_used': st.litlen_bits_used}.get(key)
            if key == 'block_types_include':
                assert want <= st.block_types, (name, key, st.block_types)
            elif key in ('stored_len', 'stored_len2'):
                assert want in st.stored_lens, (name, key, st.stored_lens[:8])
            elif key == 'blocks_min':
                assert len(st.stored_lens) >= want, (name, key, len(st.stored_lens))
            elif key == 'no_matches':
                assert not st.matches, (name, key)
            elif key == 'no_dist_code':
                assert not st.matches and st.dist_code_lengths == [[]], (name, key, st.dist_code_lengths)
            elif key == 'single_dist_code':
                assert st.matches and st.dist_code_lengths == [[1]], (name, key, st.dist_code_lengths)
            elif key == 'match':
                assert want in st.matches, (name, key, st.matches[:4])
                if want[1] < want[0]:
                    assert st.min_dist_len_ratio < 1, (name, key)
            else:
                assert got == want, (name, key, got, want)
        if depth < 8 and name.startswith('depth') and (W * depth) % 8:                     # the padding bits are set
            rows = unfilter_rows(np.frombuffer(raw, dtype=np.uint8).reshape(H, rb + 1))
            pad = rb * 8 - W * depth
            assert np.all(rows[:, -1] & ((1 << pad) - 1) == (1 << pad) - 1), name


def by_size():
    """{(H, W): [names]}: the cases of one size are decoded together in one call"""
    groups = {}
    for name, c in cases().items():
        groups.setdefault(c.label.shape, []).append(name)
    return groups


# ------------------------------------------------------------------------------------------------------------- corrupt streams

def corrupt_label():
    from boundary_ref import blobs
    return blobs(20, 30, 4, seed=17)


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """name -> (PNG file of a 20 x 30 frame with sound chunks and a damaged zlib stream, the status bit it must end in).  Each is one
    deterministic input derived from a valid stream of corrupt_label()."""
    lab = corrupt_label()
    H, W = lab.shape
    data = filtered_bytes(lab)
    good = compress(data, 'dynamic')
    toks = tokens_with_matches(data, [])
    adler = zlib.adler32(data) & 0xFFFFFFFF
    out = {}

    def add(name, stream, bit):
        out[name] = (png_around(bytes(stream), H, W), bit)

    add('truncated', good[:len(good) // 2], ST_INPUT)
    add('btype3', b'\x78\x01\x07' + struct.pack('>I', adler), ST_CODE)
    stored = bytearray(stored_stream(data, [len(data)]))
    stored[5] ^= 0x10                                       # a bit of NLEN
    add('len_nlen', stored, ST_CODE)
    add('distance_too_far', deflate_fixed(toks[:2] + [('match', 3, 5)] + toks[5:], adler=adler), ST_RANGE)
    w = BitWriter()                                         # a dynamic block whose 19 code-length codes all have length 1
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)
    add('oversubscribed', b'\x78\x01' + w.finish() + bytes(16), ST_CODE)
    add('one_match_too_many', deflate_fixed(toks + [('match', 258, 1)], adler=adler), ST_SIZE)
    bad = bytearray(good)
    bad[-1] ^= 1
    add('adler', bad, ST_ADLER)
    f5 = bytearray(data)
    f5[3 * (W + 1)] = 5
    add('filter5', compress(bytes(f5), 'dynamic'), ST_FILTER)
    add('fdict', b'\x78\x20' + good[2:], ST_HEADER)
    return out
