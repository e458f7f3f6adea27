"""Baseline-JPEG output, host side (no GPU): the numpy restatement of the encoder (tests/jpegenc_ref.py) against Pillow's files
byte for byte and against the decoder's reference (tests/jpeg_ref.py), the overlay's definition, rmem_jpeg_encode_header /
_bound / _workspace_bytes, and the argument checks of the device entry points."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as R
import jpegenc_ref as E
from png_ref import davis_palette


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def pillow_file(rgb, quality, restart_rows):
    f = io.BytesIO()
    kw = dict(restart_marker_rows=restart_rows) if restart_rows else {}
    Image.fromarray(np.asarray(rgb)).save(f, 'JPEG', quality=quality, subsampling=2, optimize=False, **kw)
    return f.getvalue()


def entropy_segment(data):
    """everything after the SOS header up to (not including) EOI"""
    at = 2
    while data[at + 1] != 0xDA:
        at += 2 + ((data[at + 2] << 8) | data[at + 3])
    at += 2 + ((data[at + 2] << 8) | data[at + 3])
    assert data[-2:] == b'\xff\xd9'
    return data[at:-2]


@functools.lru_cache(maxsize=None)
def reference(name, restart_rows):
    rgb, quality = E.case(name)
    stats = {}
    scan = E.scan_bytes(rgb, quality, restart_rows, stats)
    return scan, E.header_bytes(rgb.shape[0], rgb.shape[1], quality, restart_rows) + scan + b'\xff\xd9', stats


@pytest.mark.parametrize('restart_rows', (0, 1))
@pytest.mark.parametrize('name', E.case_names())
def test_restatement_against_pillow(name, restart_rows):
    rgb, quality = E.case(name)
    H, W, _ = rgb.shape
    scan, data, _ = reference(name, restart_rows)
    assert data == E.file_bytes(rgb, quality, restart_rows)
    theirs = pillow_file(rgb, quality, restart_rows)
    assert scan == entropy_segment(theirs)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (W, H) and im.mode == 'RGB'
    assert np.array_equal(np.array(im), np.array(Image.open(io.BytesIO(theirs))))
    J = R.parse(data)
    assert J['restart'] == restart_rows * E.geometry(H, W)['mcus_x']
    assert np.array_equal(R.decode_coefficients(J), E.coefficients(rgb, quality))


def test_the_case_set_exercises_every_feature():
    zrl = stuffed = big = dummy_dc = 0
    for name in E.case_names():
        rgb, quality = E.case(name)
        st = reference(name, 1)[2]
        zrl += st['zrl'] > 0
        stuffed += st['stuffed'] > 0
        big += st['max_size'] >= 10
        coef = E.coefficients(rgb, quality)
        dummy_dc += bool((coef[E.dummy_mask(*rgb.shape[:2]), 0] != 0).any())
        assert not coef[E.dummy_mask(*rgb.shape[:2]), 1:].any()
    assert zrl and stuffed and big and dummy_dc, (zrl, stuffed, big, dummy_dc)
    assert reference('sparse_q20_48x64', 1)[2]['zrl'] > 0 and reference('noise_q100_64x50', 1)[2]['max_size'] >= 10
    assert reference('noise_q100_64x50', 1)[2]['stuffed'] > 0
    assert E.dummy_mask(37, 53).any() and not E.dummy_mask(16, 16).any()
    assert len(R.parse(reference('tall_150x35', 1)[1])['units']) == 10          # the RST index wraps past 7
    assert b'\xff\xd0' in reference('tall_150x35', 1)[0][-400:]


def disc(H, W, cy, cx, r, label=1):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r, label, 0).astype(np.uint8)


def test_overlay_reference():
    rs = np.random.RandomState(0)
    rgb = rs.randint(1, 256, (40, 50, 3)).astype(np.uint8)                      # no black pixel of its own
    assert np.array_equal(E.overlay(rgb, np.zeros((40, 50), np.uint8)), rgb)
    lab = disc(40, 50, 20, 25, 9, 3)
    out = E.overlay(rgb, lab, 102)
    black = (out == 0).all(-1)
    inside = lab == 3
    pad = np.pad(inside, 1)
    ring = (pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]) & ~inside
    assert np.array_equal(black, ring)                                          # closed, one pixel wide, just outside
    pal = np.array(davis_palette()).reshape(256, 3)
    want = (102 * rgb[inside].astype(np.int64) + 154 * pal[3] + 128) >> 8
    assert np.array_equal(out[inside], want)
    keep = ~inside & ~ring
    assert np.array_equal(out[keep], rgb[keep])
    assert np.array_equal(E.overlay(rgb, lab, 256)[inside], rgb[inside])        # alpha 1: the contour alone
    # two touching objects: the contour lies on the smaller id's side
    two = np.zeros((10, 12), np.uint8)
    two[:, :6], two[:, 6:] = 1, 2
    o2 = E.overlay(rgb[:10, :12], two, 102)
    b2 = (o2 == 0).all(-1)
    assert b2[:, 5].all() and not b2[:, 6].any() and b2.sum() == 10
    # an object that fills the frame: image borders make no contour
    full = np.full((10, 12), 5, np.uint8)
    assert not (E.overlay(rgb[:10, :12], full, 102) == 0).all(-1).any()
    edge = np.zeros((10, 12), np.uint8)
    edge[0:4, 0:4] = 255
    be = (E.overlay(rgb[:10, :12], edge, 102) == 0).all(-1)
    assert be.sum() == 8 and be[4, :4].all() and be[:4, 4].all()


@pytest.mark.parametrize('restart_rows', (0, 1, 3))
def test_header_equals_the_reference_and_parses(lib, restart_rows):
    from rmem_ocu_amd import jpeg
    for name in E.case_names():
        rgb, quality = E.case(name)
        H, W, _ = rgb.shape
        hdr = jpeg.encode_header(H, W, quality, restart_rows)
        assert hdr == E.header_bytes(H, W, quality, restart_rows)
        assert len(hdr) <= 629
        info = jpeg.parse(hdr + E.scan_bytes(rgb, quality, restart_rows) + b'\xff\xd9')
        assert (info.height, info.width, info.components) == (H, W, 3)
        assert info.sampling == [(2, 2), (1, 1), (1, 1)]
        assert info.restart_interval == restart_rows * -(-W // 16)
        ql, qc = E.quant_tables(quality)
        assert info.quantization == {0: ql.tolist(), 1: qc.tolist()}
    assert jpeg.encode_header(480, 854) == E.header_bytes(480, 854, 90, 1)


def test_table_blob(lib):
    """the device blob: divisors 8 Q, (length << 16 | code) per symbol, restart_rows, the header"""
    tab = np.zeros(1024, np.uint32)
    n = C.c_int(0)
    assert lib.rmem_jpeg_encode_header(37, 53, 75, 2, None, 0, C.byref(n), tab.ctypes.data) == 0
    ql, qc = E.quant_tables(75)
    assert np.array_equal(tab[0:64], 8 * ql) and np.array_equal(tab[64:128], 8 * qc)
    for base, table in ((128, E.DC_LUMA), (144, E.DC_CHROMA), (160, E.AC_LUMA), (416, E.AC_CHROMA)):
        for sym, (code, length) in E.huffman_codes(table).items():
            assert tab[base + sym] == (length << 16 | code)
    assert tab[672] == 2 and tab[673] == n.value and (tab[674], tab[675]) == (37, 53)
    assert tab[676:].tobytes()[:n.value] == E.header_bytes(37, 53, 75, 2)


def test_bound_and_workspace(lib):
    for name in E.case_names():
        rgb, _ = E.case(name)
        H, W, _ = rgb.shape
        bound = lib.rmem_jpeg_encode_bound(H, W)
        assert bound == E.file_bound(H, W)
        for rr in (0, 1):
            assert len(reference(name, rr)[1]) <= bound
    assert lib.rmem_jpeg_encode_bound(8192, 8192) == E.file_bound(8192, 8192)
    f = lib.rmem_jpeg_encode_workspace_bytes
    sizes = [f(n, 40, 50) for n in (1, 2, 3, 64, 65)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert f(2, 480, 854) < f(2, 481, 854)
    for bad in ((0, 5), (5, 0), (-1, 5), (8192, 8193), (65536, 1), (1, 65536)):
        assert lib.rmem_jpeg_encode_bound(*bad) == 0 and f(1, *bad) == 0
    assert f(0, 40, 50) == 0


def test_bad_arguments_are_refused_without_a_gpu(lib):
    n = C.c_int(0)
    hdr = (C.c_ubyte * 629)()

    def header(H, W, q, rr):
        return lib.rmem_jpeg_encode_header(H, W, q, rr, hdr, 629, C.byref(n), None)

    assert header(37, 53, 75, 1) == 0
    for args, reason in (((37, 53, 0, 1), b'quality'), ((37, 53, 101, 1), b'quality'), ((0, 53, 75, 1), b'1..65535'),
                         ((37, 65536, 75, 1), b'1..65535'), ((8192, 8193, 75, 1), b'2^26'), ((16, 65535, 75, 16), b'restart_rows'),
                         ((37, 53, 75, -1), b'restart_rows')):
        assert header(*args) != 0
        assert reason in lib.rmem_last_error_string(), (args, lib.rmem_last_error_string())
    assert header(16, 65520, 75, 16) == 0 and header(16, 65521, 75, 16) != 0      # 4095 and 4096 MCUs per row: DRI 65520, 65536
    assert header(16, 65535, 75, 15) == 0 and header(16, 65535, 75, 0) == 0
    enc = lib.rmem_jpeg_encode_rgb8
    for H, W, reason in ((0, 50, b'1..65535'), (40, 65536, b'1..65535'), (8192, 8193, b'2^26')):
        assert enc(16, None, None, 102, 1, H, W, 16, 16, 16, 16, None) != 0
        assert reason in lib.rmem_last_error_string()
    assert enc(16, None, None, 102, 0, 40, 50, 16, 16, 16, 16, None) != 0 and b'frames' in lib.rmem_last_error_string()
    for args in ((None, None, None, 102, 1, 40, 50, 16, 16, 16, 16, None), (16, None, None, 102, 1, 40, 50, None, 16, 16, 16, None),
                 (16, None, None, 102, 1, 40, 50, 16, None, 16, 16, None), (16, None, None, 102, 1, 40, 50, 16, 16, None, 16, None),
                 (16, None, None, 102, 1, 40, 50, 16, 16, 16, None, None), (16, 16, None, 102, 1, 40, 50, 16, 16, 16, 16, None)):
        assert enc(*args) != 0
        assert b'null' in lib.rmem_last_error_string()
    assert enc(16, 16, 16, 257, 1, 40, 50, 16, 16, 16, 16, None) != 0 and b'alpha256' in lib.rmem_last_error_string()
    ov = lib.rmem_overlay_rgb8
    assert ov(16, None, 16, 102, 1, 40, 50, 16, None) != 0 and b'null' in lib.rmem_last_error_string()
    assert ov(16, 16, 16, -1, 1, 40, 50, 16, None) != 0 and b'alpha256' in lib.rmem_last_error_string()
    assert ov(16, 16, 16, 102, 1, 8192, 8193, 16, None) != 0 and b'2^26' in lib.rmem_last_error_string()


def test_python_refuses_bad_settings_and_host_tensors():
    import torch
    from rmem_ocu_amd import evaluator, jpeg
    from rmem_ocu_amd._lib import RmemError
    for args, reason in (((37, 53, 0), 'quality'), ((37, 53, 101), 'quality'), ((0, 53), '1..65535'), ((37, 65536), '1..65535'),
                         ((8192, 8193), '2\\^26'), ((16, 65535, 90, 16), 'restart_rows'), ((37.5, 53), 'integer')):
        with pytest.raises(RmemError, match=reason):
            jpeg.encode_header(*args)
    rgb = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for fn in (jpeg.encode_files, jpeg.encode_rgb_stack):
        with pytest.raises(RmemError, match='device'):
            fn(rgb)
        with pytest.raises(RmemError, match='device'):
            fn(rgb, lab)
    with pytest.raises(RmemError, match='device'):
        jpeg.overlay(rgb, lab)
    with pytest.raises(RmemError, match='device'):
        evaluator.save_overlays(rgb, lab, ['a', 'b'])

