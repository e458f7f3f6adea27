"""A numpy / Python restatement of the palette-PNG format of include/rmem.h (rmem_png_encode_labels): the tests' reference for the
device encoder and for rmem_ocu_amd.png.wrap.  Independent of rmem_ocu_amd.

A frame's zlib stream: 78 01, one fixed-Huffman DEFLATE block (BFINAL = 1, BTYPE = 01) over the Up-filtered rows, the end-of-block
code, zero bits to the byte boundary, the Adler-32 of the filtered bytes big-endian.  Every row (filter byte 2, then the W
differences to the row above, the row above row 0 being zero) is cut into maximal runs of equal bytes; a run of value v and length
L is: literal v; rem = L - 1; while rem >= 3 a match of distance 1 and length min(rem, 258); then rem literals v.
Runs are found with numpy, tokens are written one by one in Python: a blob map costs milliseconds, noise about a second per
100,000 pixels.
"""
import struct
import zlib

import numpy as np

# RFC 1951 3.2.5: (first length, extra bits) of the length codes 257..285
LENGTH_CODES = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2),
                (27, 2), (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5),
                (227, 5), (258, 0)]


def davis_palette():
    """the 256-colour DAVIS palette as 768 ints (the bit-reversal colour map)"""
    pal = []
    for i in range(256):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        pal += rgb
    return pal


def zlib_bound(H, W):
    return 2 + (3 + 9 * (W + 1) * H + 7 + 7) // 8 + 4


def filtered(label, lut=None):
    """uint8 [H, W + 1]: per row the filter type 2, then label[y] - label[y - 1] mod 256"""
    lab = np.asarray(label, dtype=np.uint8)
    if lut is not None:
        lab = np.asarray(lut, dtype=np.uint8)[lab]
    H, W = lab.shape
    out = np.empty((H, W + 1), dtype=np.uint8)
    out[:, 0] = 2
    above = np.zeros_like(lab)
    above[1:] = lab[:-1]
    out[:, 1:] = lab - above
    return out


def fixed_code(sym):
    """RFC 1951 3.2.6: (code, bits) of literal / length symbol sym; the code goes out most significant bit first"""
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def length_code(t):
    """(symbol, extra bits, extra value) of match length t"""
    if t == 258:
        return 285, 0, 0
    for i in range(len(LENGTH_CODES) - 2, -1, -1):
        first, extra = LENGTH_CODES[i]
        if t >= first:
            return 257 + i, extra, t - first
    raise ValueError(t)


def run_tokens(v, L):
    """tokens of one run: ('lit', v) and ('match', length)"""
    toks = [('lit', v)]
    rem = L - 1
    while rem >= 3:
        t = min(rem, 258)
        toks.append(('match', t))
        rem -= t
    toks += [('lit', v)] * rem
    return toks


def row_runs(row):
    """[(value, length)] of the maximal runs of a 1-D uint8 array"""
    row = np.asarray(row)
    starts = np.concatenate(([0], np.flatnonzero(row[1:] != row[:-1]) + 1, [row.size]))
    return [(int(row[s]), int(e - s)) for s, e in zip(starts[:-1], starts[1:])]


def tokens(filt):
    out = []
    for row in filt:
        for v, L in row_runs(row):
            out += run_tokens(v, L)
    return out


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

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
        self.bits(int(format(code, '0%db' % n)[::-1], 2), n)

    def finish(self):
        if self.n:
            self.buf.append(self.acc & 255)
            self.acc = self.n = 0
        return bytes(self.buf)


def deflate_block(toks):
    w = BitWriter()
    w.bits(1, 1)                      # BFINAL
    w.bits(1, 2)                      # BTYPE = 01
    for kind, x in toks:
        if kind == 'lit':
            w.huffman(*fixed_code(x))
        else:
            sym, extra, ev = length_code(x)
            w.huffman(*fixed_code(sym))
            w.bits(ev, extra)
            w.huffman(0, 5)           # distance code 0 = distance 1
    w.huffman(*fixed_code(256))
    return w.finish()


def adler32(data):
    """RFC 1950, byte by byte in chunks small enough for int64 sums"""
    a, b = 1, 0
    d = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64)
    for i in range(0, d.size, 4096):
        c = d[i:i + 4096]
        n = c.size
        b = (b + n * a + int((np.arange(n, 0, -1, dtype=np.int64) * c).sum())) % 65521
        a = (a + int(c.sum())) % 65521
    return b << 16 | a


def zlib_stream(label, lut=None):
    filt = filtered(label, lut)
    return b'\x78\x01' + deflate_block(tokens(filt)) + struct.pack('>I', adler32(filt.tobytes()))


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def wrap(stream, H, W, palette=None):
    """a complete PNG file around one zlib stream: signature, IHDR (8 bit, colour type 3), PLTE, IDAT, IEND"""
    pal = bytes(davis_palette() if palette is None else palette)
    assert len(pal) == 768
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 3, 0, 0, 0)) + chunk(b'PLTE', pal)
            + chunk(b'IDAT', bytes(stream)) + chunk(b'IEND', b''))


def png_file(label, lut=None, palette=None):
    lab = np.asarray(label)
    return wrap(zlib_stream(lab, lut), lab.shape[0], lab.shape[1], palette)


def squeeze_lut(squeeze_idx):
    """what save_mask's un-squeeze loop does to every label value 0..255, as a 256-entry table"""
    mask = np.arange(256, dtype=np.uint8)
    out = np.zeros_like(mask)
    for idx in range(1, len(squeeze_idx)):
        out += ((mask == idx) * squeeze_idx[idx]).astype(np.uint8)
    return out


RUN_WIDTHS = (1, 2, 3, 4, 63, 64, 65, 259, 260, 261, 262, 517, 518)


def case_names():
    """the label maps both test tiers run: the smallest shapes at which the format or an encoder can go wrong"""
    names = ['run_v%d_w%d' % (v, w) for v in (1, 2) for w in RUN_WIDTHS]
    return names + ['symbols_5x7', 'alternating_rows', 'void_3x600', 'noise_64x200', 'noise9_64x200', 'blobs_97x131', 'blobs_33x129', 'blobs_480x854',
                    'blobs_1080x1920']


def case(name):
    """uint8 [H, W] label map of a named case"""
    from boundary_ref import blobs
    if name.startswith('run_v'):
        v, w = name[5:].split('_w')
        # value 1: per row a run of W equal bytes after the filter byte (row 0: ones, row 1: zeros), L - 1 = W - 1;
        # value 2: row 0's run merges with the filter byte 2 and is W + 1 long
        return np.full((2, int(w)), int(v), dtype=np.uint8)
    if name == 'symbols_5x7':          # 8- and 9-bit literals on both sides of 143 / 144
        return np.array([0, 143, 144, 255], dtype=np.uint8)[np.random.RandomState(7).randint(0, 4, (5, 7))]
    if name == 'alternating_rows':     # Up differences 1 and 255
        lab = np.zeros((6, 70), dtype=np.uint8)
        lab[1::2] = 1
        return lab
    if name == 'void_3x600':
        return np.full((3, 600), 255, dtype=np.uint8)
    if name == 'noise_64x200':         # every byte its own run (almost): the worst case of the bound
        return np.random.RandomState(11).randint(0, 256, (64, 200)).astype(np.uint8)
    if name == 'noise9_64x200':        # Up differences uniform in 144..255, neighbours unequal: every byte a 9-bit literal.  Uniform
        rs = np.random.RandomState(12)  # labels give uniform differences, 144 of 256 of them 8-bit literals: 0.937 of the bound
        d = rs.randint(144, 256, (64, 200))
        for x in range(1, 200):
            same = d[:, x] == d[:, x - 1]
            d[same, x] = 144 + (d[same, x] - 144 + 1) % 112
        return (np.cumsum(d, axis=0) % 256).astype(np.uint8)
    if name == 'blobs_97x131':
        return blobs(97, 131, 5, seed=1)
    if name == 'blobs_33x129':
        return blobs(33, 129, 5, seed=2)
    if name == 'blobs_480x854':
        return blobs(480, 854, 11, seed=3)
    if name == 'blobs_1080x1920':
        return blobs(1080, 1920, 6, seed=4)
    raise KeyError(name)
