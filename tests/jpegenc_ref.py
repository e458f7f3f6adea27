"""A numpy / Python restatement of baseline JPEG encoding as libjpeg-turbo does it at 4:2:0 with the standard tables (the tests'
reference for rmem_jpeg_encode_* and rmem_overlay_rgb8, include/rmem.h).  Independent of rmem_ocu_amd; sequential and slow, meant
for small images.

  colour      jccolor.c, 16-bit fixed point
  sampling    Y 2x2, Cb and Cr 1x1; luma replicated right / down to whole blocks; chroma replicated right at full resolution and
              down by at most one row (to an even height), averaged 2x2 with the bias 1, 2, 1, 2 ..., then its rows replicated
  FDCT        jfdctint.c (ISLOW) on sample - 128, rows first; quantised with d = 8 Q, q = (|c| + (d >> 1)) / d, sign restored
  dummies     blocks of the MCU grid beyond a component's real blocks: ACs zero, DC = the DC of the preceding block of the MCU
  entropy     Annex K's four tables; DC difference per component, reset at every restart interval; ZRL, EOB; an interval is padded
              with 1-bits, every 0xFF data byte is followed by 0x00, RSTm (m = interval index mod 8) between intervals
  overlay     the project's integer overlay: contour where a 4-neighbour carries a larger label, else palette blend, else unchanged
"""
import functools
import struct

import numpy as np

from jpeg_ref import FIX, ZIGZAG

Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)


def _runs(*spans):
    return [v for a, b in spans for v in range(a, b + 1)]


# Annex K.3: (number of codes of each length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A]
           + _runs((0x16, 0x1A), (0x25, 0x2A), (0x34, 0x3A), (0x43, 0x4A), (0x53, 0x5A), (0x63, 0x6A), (0x73, 0x7A), (0x83, 0x8A),
                   (0x92, 0x9A), (0xA2, 0xAA), (0xB2, 0xBA), (0xC2, 0xCA), (0xD2, 0xDA), (0xE1, 0xEA), (0xF1, 0xFA)))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
              0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A]
             + _runs((0x26, 0x2A), (0x35, 0x3A), (0x43, 0x4A), (0x53, 0x5A), (0x63, 0x6A), (0x73, 0x7A), (0x82, 0x8A), (0x92, 0x9A),
                     (0xA2, 0xAA), (0xB2, 0xBA), (0xC2, 0xCA), (0xD2, 0xDA), (0xE2, 0xEA), (0xF2, 0xFA)))


def huffman_codes(table):
    """symbol -> (code, length), Annex C"""
    counts, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_tables(quality):
    """(luma, chroma) in natural order: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline"""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (Q_LUMA, Q_CHROMA))


def geometry(H, W):
    g = dict(H=H, W=W, mcus_x=-(-W // 16), mcus_y=-(-H // 16))
    g['cw'], g['ch'] = [W, -(-W // 2), -(-W // 2)], [H, -(-H // 2), -(-H // 2)]
    g['wib'], g['hib'] = [-(-v // 8) for v in g['cw']], [-(-v // 8) for v in g['ch']]
    return g


def ycc(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _grow(a, rows, cols):
    """replicate the last column up to `cols` columns, then the last row up to `rows` rows"""
    a = np.concatenate([a] + [a[:, -1:]] * (cols - a.shape[1]), axis=1) if cols > a.shape[1] else a
    return np.concatenate([a] + [a[-1:]] * (rows - a.shape[0]), axis=0) if rows > a.shape[0] else a


def sample_planes(rgb):
    """[Y, Cb, Cr] sample planes of 8 hib x 8 wib samples each (the real blocks only)"""
    H, W, _ = rgb.shape
    g = geometry(H, W)
    y, cb, cr = ycc(rgb)
    planes = [_grow(y, 8 * g['hib'][0], 8 * g['wib'][0])]
    for c in (cb, cr):
        full = _grow(c, H + (H & 1), 16 * g['wib'][1])
        bias = np.tile(np.array([1, 2]), full.shape[1] // 4)[None, :]
        down = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
        planes.append(_grow(down, 8 * g['hib'][1], down.shape[1]))
    return planes


def _fdct_1d(x, first):
    """one jfdctint.c pass over the last axis: first = the row pass (results scaled up by PASS1_BITS)"""
    F = FIX
    d = [x[..., n] for n in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15

    def ds(v, k):
        return (v + (1 << (k - 1))) >> k

    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else ds(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else ds(t10 - t11, 2)
    z1 = (t12 + t13) * F['c']
    o[2] = ds(z1 + t13 * F['d'], n)
    o[6] = ds(z1 - t12 * F['h'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['f']
    t4, t5, t6, t7 = t4 * F['a'], t5 * F['j'], t6 * F['l'], t7 * F['g']
    z1, z2, z3, z4 = -z1 * F['e'], -z2 * F['k'], -z3 * F['i'] + z5, -z4 * F['b'] + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(plane, q):
    """[hb * 8, wb * 8] samples -> int64 [hb, wb, 64] quantised coefficients in natural order"""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128              # [hb, wb, row, col]
    p1 = _fdct_1d(b, True)
    p2 = np.swapaxes(_fdct_1d(np.swapaxes(p1, 2, 3), False), 2, 3)
    c = p2.reshape(hb, wb, 64)
    d = (8 * q)[None, None, :]
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(rgb, quality):
    """int16 [total_blocks, 64], natural order, DC values: the layout of jpeg_ref.decode_coefficients (component planes of the whole
    MCU grid back to back), dummy blocks filled by jccoefct.c's rule"""
    H, W, _ = rgb.shape
    g = geometry(H, W)
    ql, qc = quant_tables(quality)
    out = []
    for ci, (plane, q) in enumerate(zip(sample_planes(rgb), (ql, qc, qc))):
        s = 2 if ci == 0 else 1
        real = fdct_quant(plane, q)
        grid = np.zeros((g['mcus_y'] * s, g['mcus_x'] * s, 64), np.int64)
        hib, wib = g['hib'][ci], g['wib'][ci]
        grid[:hib, :wib] = real
        if wib < grid.shape[1]:                                                # a dummy column: the block to its left
            grid[:hib, wib, 0] = grid[:hib, wib - 1, 0]
        if hib < grid.shape[0]:                                                # a dummy row: the last block of the MCU's row above
            grid[hib, :, 0] = np.repeat(grid[hib - 1, 1::2, 0], 2)
        out.append(grid.reshape(-1, 64))
    return np.concatenate(out).astype(np.int16)


def dummy_mask(H, W):
    """bool [total_blocks]: which blocks of `coefficients` are dummies"""
    g = geometry(H, W)
    m = np.zeros((g['mcus_y'] * 2, g['mcus_x'] * 2), bool)
    m[g['hib'][0]:] = True
    m[:, g['wib'][0]:] = True
    return np.concatenate([m.ravel(), np.zeros(2 * g['mcus_y'] * g['mcus_x'], bool)])


def scan_blocks(H, W):
    """per MCU in scan order the six (component, index into `coefficients`) of its blocks"""
    g = geometry(H, W)
    mx, my = g['mcus_x'], g['mcus_y']
    base = [0, 4 * mx * my, 5 * mx * my]
    for r in range(my):
        for c in range(mx):
            yield [(0, base[0] + (2 * r + k // 2) * 2 * mx + 2 * c + k % 2) for k in range(4)] + [(1, base[1] + r * mx + c),
                                                                                                   (2, base[2] + r * mx + c)]


class _BitSink:
    def __init__(self):
        self.acc, self.n, self.symbols = 0, 0, []

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def bytes(self):
        pad = -self.n % 8
        v = (self.acc << pad) | ((1 << pad) - 1)
        return v.to_bytes((self.n + pad) // 8, 'big') if self.n else b''


def _size(v):
    return int(abs(int(v))).bit_length()


def _encode_block(sink, blk, pred, dc, ac, stats):
    diff = int(blk[0]) - pred
    s = _size(diff)
    sink.put(*dc[s])
    sink.put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
    stats['max_size'] = max(stats['max_size'], s)
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            sink.put(*ac[0xF0])
            stats['zrl'] += 1
            run -= 16
        s = _size(v)
        stats['max_size'] = max(stats['max_size'], s)
        sink.put(*ac[(run << 4) | s])
        sink.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        run = 0
    if run:
        sink.put(*ac[0x00])


def scan_bytes(rgb, quality, restart_rows=1, stats=None):
    """the entropy-coded segment: everything after the SOS header up to (not including) EOI"""
    H, W, _ = rgb.shape
    g = geometry(H, W)
    coef = coefficients(rgb, quality)
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA), huffman_codes(AC_CHROMA)]
    stats = stats if stats is not None else {}
    stats.update(zrl=0, max_size=0, stuffed=0)
    per = restart_rows * g['mcus_x'] if restart_rows else g['mcus_x'] * g['mcus_y']
    out, sink, pred = bytearray(), _BitSink(), [0, 0, 0]
    units = 0
    for m, blocks in enumerate(scan_blocks(H, W)):
        if m and m % per == 0:
            data = sink.bytes()
            stats['stuffed'] += data.count(b'\xff')
            out += data.replace(b'\xff', b'\xff\x00') + bytes([0xFF, 0xD0 + units % 8])
            units += 1
            sink, pred = _BitSink(), [0, 0, 0]
        for ci, idx in blocks:
            _encode_block(sink, coef[idx], pred[ci], dc[ci], ac[ci], stats)
            pred[ci] = int(coef[idx][0])
    data = sink.bytes()
    stats['stuffed'] += data.count(b'\xff')
    return bytes(out + data.replace(b'\xff', b'\xff\x00'))


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack('>H', len(body) + 2) + bytes(body)


def header_bytes(H, W, quality=90, restart_rows=1):
    """SOI, APP0 (JFIF 1.01), two DQT, SOF0, four DHT, DRI if restart_rows, SOS"""
    assert 1 <= H <= 65535 and 1 <= W <= 65535
    ql, qc = quant_tables(quality)
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for tq, q in enumerate((ql, qc)):
        out += _segment(0xDB, bytes([tq]) + bytes(int(v) for v in q[ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + struct.pack('>HH', H, W) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (counts, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(counts) + bytes(vals))
    if restart_rows:
        dri = restart_rows * geometry(H, W)['mcus_x']
        assert dri <= 65535
        out += _segment(0xDD, struct.pack('>H', dri))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def file_bytes(rgb, quality=90, restart_rows=1):
    H, W, _ = rgb.shape
    return header_bytes(H, W, quality, restart_rows) + scan_bytes(rgb, quality, restart_rows) + b'\xff\xd9'


def file_bound(H, W):
    """rmem_jpeg_encode_bound: a block takes at most 22 + 63 * 26 bits (DC: an 11-bit code + 11 bits; AC: a 16-bit code + 10 bits),
    every byte may be stuffed, an interval pads to a byte and is followed by a 2-byte marker (at most one interval per MCU row),
    plus the longest header (with DRI) and EOI"""
    g = geometry(H, W)
    return len(header_bytes(16, 16, 90, 1)) + 2 * (g['mcus_x'] * g['mcus_y'] * 6 * 208) + 4 * g['mcus_y'] + 2


def overlay(rgb, labels, alpha256=102, palette=None):
    """uint8 [H, W, 3]: black where a 4-neighbour inside the image carries a larger label, else (label != 0) the palette blend
    (a rgb + (256 - a) palette + 128) >> 8, else the pixel"""
    from png_ref import davis_palette
    pal = np.asarray(davis_palette() if palette is None else palette, dtype=np.int64).reshape(256, 3)
    lab = np.asarray(labels, dtype=np.int64)
    H, W = lab.shape
    pad = np.full((H + 2, W + 2), -1, np.int64)
    pad[1:-1, 1:-1] = lab
    m = np.max(np.stack([pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]]), axis=0)
    blend = (alpha256 * rgb.astype(np.int64) + (256 - alpha256) * pal[lab] + 128) >> 8
    out = np.where((lab != 0)[..., None], blend, rgb.astype(np.int64))
    out[m > lab] = 0
    return out.astype(np.uint8)


def _smooth(rs, H, W, amp=40):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], -1)
    return np.clip(base + rs.randint(-amp, amp + 1, (H, W, 3)), 0, 255).astype(np.uint8)


def _noise_q100(rs, H, W):
    a = rs.randint(0, 256, (H, W, 3))
    a[:8] = np.where(((np.arange(W) // 8) % 2 == 0)[None, :, None], 0, 255)       # black / white blocks: DC differences of size 11
    a[8:16, :, 1] = np.where(rs.randint(0, 2, (8, W)) > 0, 255, 0)
    return a.astype(np.uint8)


def _sparse(rs, H, W):
    a = np.full((H, W, 3), 120, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    a[:16, :32] += (40 * (-1) ** (xx[:16, :32] + yy[:16, :32]))[..., None]        # the last zig-zag position: three ZRLs
    a[16:32, 16:] += (45 * (-1) ** xx[16:32, 16:])[..., None]                     # horizontal frequency 7 alone
    a[32:, :48] += (45 * (-1) ** yy[32:, :48])[..., None]
    a[40:44, 50:60] += rs.randint(-3, 4, (4, 10, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


_CASES = {
    'one_mcu_16x16': (16, 16, 90, _smooth),
    'odd_37x53': (37, 53, 75, _smooth),
    'short_9x100': (9, 100, 85, _smooth),
    'narrow_33x17': (33, 17, 30, _smooth),
    'tall_150x35': (150, 35, 60, _smooth),
    'wide_16x1300': (16, 1300, 90, _smooth),
    'noise_q100_64x50': (64, 50, 100, _noise_q100),
    'sparse_q20_48x64': (48, 64, 20, _sparse),
    'flat_32x32': (32, 32, 90, lambda rs, H, W: np.full((H, W, 3), (200, 60, 30), np.uint8)),
}


def case_names():
    return list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(rgb uint8 [H, W, 3] (read-only), quality)"""
    H, W, quality, make = _CASES[name]
    rgb = make(np.random.RandomState(sum(name.encode())), H, W)
    rgb.setflags(write=False)
    return rgb, quality
