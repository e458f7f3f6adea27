"""A numpy restatement of baseline JPEG decoding as libjpeg-turbo does it (the tests' reference for rmem_jpeg_*).

Sequential and slow; meant for small images.  Covers what the device decoder covers: 8-bit Huffman, one scan, grayscale or
YCbCr at 4:4:4 / 4:2:2 (h2v1) / 4:2:0 (h2v2), restart intervals.  Stages:
  decode_coefficients: Huffman decode -> int16 [total_blocks, 64] natural order, DC values, component planes back to back;
  idct_islow:          jidctint.c (CONST_BITS 13, PASS1_BITS 2, post-IDCT range limit) -> per-component sample planes;
  to_rgb:              jdsample.c fancy upsampling (replication when downsampled_width <= 2) + jdcolor.c YCbCr->RGB.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])


class DecodeError(ValueError):
    pass


def parse(data: bytes) -> dict:
    assert data[:2] == b'\xff\xd8'
    pos, q, huff, dri, sof = 2, {}, {}, 0, None
    while True:
        while data[pos] != 0xFF:
            pos += 1
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        ln = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2:pos + ln]
        pos += ln
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq:
                    vals = [(seg[i + 1 + 2 * k] << 8) | seg[i + 2 + 2 * k] for k in range(64)]
                else:
                    vals = list(seg[i + 1:i + 65])
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = vals
                q[tq] = t
                i += 1 + 64 * (2 if pq else 1)
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                n = sum(counts)
                vals = list(seg[i + 17:i + 17 + n])
                table, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[(tc, th)] = table
                i += 17 + n
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m in (0xC0, 0xC1):
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            comps = [dict(id=seg[6 + 3 * c], h=seg[7 + 3 * c] >> 4, v=seg[7 + 3 * c] & 15, tq=seg[8 + 3 * c]) for c in range(nc)]
            sof = dict(width=w, height=h, comps=comps)
        elif m == 0xDA:
            ns = seg[0]
            for k in range(ns):
                sof['comps'][k]['td'] = seg[2 + 2 * k] >> 4
                sof['comps'][k]['ta'] = seg[2 + 2 * k] & 15
            break
    # entropy-coded segment: strip stuffing, split at RSTn
    units, cur, i = [], bytearray(), pos
    while True:
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nx = data[i + 1]
        if nx == 0x00:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= nx <= 0xD7:
            units.append(bytes(cur))
            cur = bytearray()
            i += 2
        elif nx == 0xFF:
            i += 1
        else:
            break
    units.append(bytes(cur))
    sof.update(quant=q, huff=huff, restart=dri, units=units)
    gray = len(sof['comps']) == 1
    if gray:
        sof['comps'][0]['h'] = sof['comps'][0]['v'] = 1
    hmax = max(c['h'] for c in sof['comps'])
    vmax = max(c['v'] for c in sof['comps'])
    sof['hmax'], sof['vmax'] = hmax, vmax
    sof['mcus_x'] = -(-sof['width'] // (8 * hmax))
    sof['mcus_y'] = -(-sof['height'] // (8 * vmax))
    b0 = 0
    for c in sof['comps']:
        c['bw'], c['bh'] = sof['mcus_x'] * c['h'], sof['mcus_y'] * c['v']
        c['block0'] = b0
        b0 += c['bw'] * c['bh']
        c['dw'] = -(-sof['width'] * c['h'] // hmax)
        c['dh'] = -(-sof['height'] * c['v'] // vmax)
    sof['total_blocks'] = b0
    return sof


class _Bits:
    def __init__(self, data: bytes):
        self.v = int.from_bytes(data + b'\0' * 8, 'big')
        self.n = (len(data) + 8) * 8
        self.p = 0

    def get(self, k):
        if k == 0:
            return 0
        r = (self.v >> (self.n - self.p - k)) & ((1 << k) - 1)
        self.p += k
        return r

    def decode(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get(1)
            s = table.get((length, code))
            if s is not None:
                return s
        raise DecodeError('invalid Huffman code')


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_coefficients(J: dict) -> np.ndarray:
    """int16 [total_blocks, 64], natural order, DC values; component planes of comp['bw'] x comp['bh'] blocks back to back."""
    coef = np.zeros((J['total_blocks'], 64), np.int64)
    comps = J['comps']
    order = [(ci, k) for ci, c in enumerate(comps) for k in range(c['h'] * c['v'])]
    mcus = J['mcus_x'] * J['mcus_y']
    per_unit = J['restart'] or mcus
    if len(J['units']) != -(-mcus // per_unit):
        raise DecodeError('restart marker count')
    for u, data in enumerate(J['units']):
        bits = _Bits(data)
        pred = [0] * len(comps)
        for mcu in range(u * per_unit, min(mcus, (u + 1) * per_unit)):
            my, mx = divmod(mcu, J['mcus_x'])
            for ci, sub in order:
                c = comps[ci]
                row = my * c['v'] + sub // c['h']
                col = mx * c['h'] + sub % c['h']
                blk = coef[c['block0'] + row * c['bw'] + col]
                s = bits.decode(J['huff'][(0, c['td'])])
                pred[ci] += _extend(bits.get(s), s)
                blk[0] = pred[ci]
                k = 1
                while k < 64:
                    rs = bits.decode(J['huff'][(1, c['ta'])])
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        if k > 63:
                            raise DecodeError('coefficient index')
                        blk[ZIGZAG[k]] = _extend(bits.get(s), s)
                        k += 1
                    elif r == 15:
                        k += 16
                        if k > 63:
                            raise DecodeError('coefficient index')
                    else:
                        break
    return coef.astype(np.int16)


FIX = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)


def _idct_1d(x, shift):
    """x [..., 8] int64 -> [..., 8], one jidctint.c pass with DESCALE by `shift`."""
    F = FIX
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., n] for n in range(8))
    z1 = (i2 + i6) * F['c']
    tmp2 = z1 + i6 * -F['h']
    tmp3 = z1 + i2 * F['d']
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = t0 + tmp3, t0 - tmp3, t1 + tmp2, t1 - tmp2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F['f']
    a0, a1, a2, a3 = a0 * F['a'], a1 * F['j'], a2 * F['l'], a3 * F['g']
    z1, z2 = z1 * -F['e'], z2 * -F['k']
    z3 = z3 * -F['i'] + z5
    z4 = z4 * -F['b'] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    rnd = 1 << (shift - 1)
    out = [tmp10 + a3, tmp11 + a2, tmp12 + a1, tmp13 + a0, tmp13 - a0, tmp12 - a1, tmp11 - a2, tmp10 - a3]
    return np.stack([(o + rnd) >> shift for o in out], axis=-1)


def _range_limit(v):
    x = v & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)


def idct_islow(J: dict, coef: np.ndarray) -> list:
    """per component uint8 planes [bh*8, bw*8]."""
    planes = []
    for c in J['comps']:
        n = c['bw'] * c['bh']
        blocks = coef[c['block0']:c['block0'] + n].astype(np.int64) * J['quant'][c['tq']][None, :]
        b = blocks.reshape(n, 8, 8)                                  # [blk, row, col]
        p1 = _idct_1d(np.swapaxes(b, 1, 2), 11)                      # columns: [blk, col, row]
        p2 = _idct_1d(np.swapaxes(p1, 1, 2), 18)                     # rows:    [blk, row, col]
        s = _range_limit(p2).reshape(c['bh'], c['bw'], 8, 8).transpose(0, 2, 1, 3).reshape(c['bh'] * 8, c['bw'] * 8)
        planes.append(s)
    return planes


def _upsample(plane, c, hmax, vmax, H, W):
    dw, dh = c['dw'], c['dh']
    x = plane[:dh, :dw].astype(np.int64)
    if c['h'] == hmax and c['v'] == vmax:
        return x[:H, :W]
    if dw <= 2:                                                      # jdsample.c: plain replication
        x = np.repeat(x, 2, axis=1)
        if vmax == 2:
            x = np.repeat(x, 2, axis=0)
        return x[:H, :W]
    if vmax == 2:
        up = np.concatenate([x[:1], x[:-1]], 0)
        dn = np.concatenate([x[1:], x[-1:]], 0)
        cs = np.empty((2 * dh, dw), np.int64)
        cs[0::2] = 3 * x + up
        cs[1::2] = 3 * x + dn
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out = np.empty((2 * dh, 2 * dw), np.int64)
        out[:, 0::2] = (3 * cs + left + 8) >> 4
        out[:, 1::2] = (3 * cs + right + 7) >> 4
    else:
        left = np.concatenate([x[:, :1], x[:, :-1]], 1)
        right = np.concatenate([x[:, 1:], x[:, -1:]], 1)
        out = np.empty((dh, 2 * dw), np.int64)
        out[:, 0::2] = (3 * x + left + 1) >> 2
        out[:, 1::2] = (3 * x + right + 2) >> 2
    return out[:H, :W]


def to_rgb(J: dict, planes: list) -> np.ndarray:
    H, W = J['height'], J['width']
    y = planes[0][:H, :W].astype(np.int64)
    if len(J['comps']) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb = _upsample(planes[1], J['comps'][1], J['hmax'], J['vmax'], H, W) - 128
    cr = _upsample(planes[2], J['comps'][2], J['hmax'], J['vmax'], H, W) - 128
    half = 1 << 15
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-46802 * cr - 22554 * cb + half) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    J = parse(data)
    return to_rgb(J, idct_islow(J, decode_coefficients(J).astype(np.int64)))
