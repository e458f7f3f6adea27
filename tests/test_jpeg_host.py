"""JPEG ingest, host side (no GPU): rmem_jpeg_parse / rmem_jpeg_pack against Pillow, the rejection of unsupported files, and
the numpy restatement of the decoder (tests/jpeg_ref.py) against Pillow bit for bit."""
import ctypes
import io

import numpy as np
import pytest

PIL = pytest.importorskip('PIL')
from PIL import Image, JpegImagePlugin  # noqa: E402

import jpeg_ref  # noqa: E402

SAMPLING = {'L': None, '444': 0, '422': 1, '420': 2}


def encode(a, mode, quality=90, **kw):
    b = io.BytesIO()
    if mode == 'L':
        Image.fromarray(a[..., 0] if a.ndim == 3 else a).save(b, 'JPEG', quality=quality, **kw)
    else:
        Image.fromarray(a).save(b, 'JPEG', quality=quality, subsampling=SAMPLING[mode], **kw)
    return b.getvalue()


def image(h, w, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 4) % 256], -1)
    return np.clip(smooth + rs.randint(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not __import__('os').path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


CASES = [('L', {}), ('444', {}), ('422', {}), ('420', {}), ('420', {'optimize': True}), ('444', {'optimize': True}),
         ('420', {'restart_marker_blocks': 5}), ('422', {'restart_marker_rows': 1}), ('L', {'restart_marker_rows': 2})]


@pytest.mark.parametrize('mode,kw', CASES)
def test_parse_agrees_with_pillow(lib, mode, kw):
    from rmem_ocu_amd import jpeg
    d = encode(image(37, 61), mode, 85, **kw)
    im = Image.open(io.BytesIO(d))
    info = jpeg.parse(d)
    assert (info.width, info.height) == im.size
    assert info.components == (1 if im.mode == 'L' else 3)
    assert [(h, v) for (_, h, v, _) in im.layer] == info.sampling
    assert [t for (_, _, _, t) in im.layer] == info.quant_ids
    samp = {((1, 1), (1, 1), (1, 1)): 0, ((2, 1), (1, 1), (1, 1)): 1, ((2, 2), (1, 1), (1, 1)): 2}
    assert samp.get(tuple(info.sampling), -1) == JpegImagePlugin.get_sampling(im)
    assert {k: list(v) for k, v in im.quantization.items()} == info.quantization
    hmax = max(h for h, _ in info.sampling) if info.components == 3 else 1
    mcus_x = -(-info.width // (8 * hmax))
    expect = kw.get('restart_marker_blocks', 0) or kw.get('restart_marker_rows', 0) * mcus_x
    assert info.restart_interval == expect
    assert d[info.scan_range[1]:info.scan_range[1] + 2] == b'\xff\xd9'


def test_pack_strips_stuffing_and_restart_markers(lib):
    from rmem_ocu_amd import jpeg
    d = encode(image(40, 72, 3), '420', 95, restart_marker_blocks=4)
    J = jpeg_ref.parse(d)
    p = jpeg.PackedJpegs([d])
    desc = p.descs[0]
    buf = p.buf.numpy()
    assert desc.nunits == len(J['units']) and desc.restart_mcus == 4
    tab = buf[desc.offset:desc.offset + 8 * (desc.nunits + 1)].view(np.uint32).reshape(-1, 2)
    data = buf[desc.offset + desc.data_off:].tobytes()
    assert tab[-1, 0] == desc.data_bits == 8 * sum(len(u) for u in J['units'])
    for u, ref in enumerate(J['units']):
        a = tab[u, 0] // 8
        assert data[a:a + len(ref)] == ref
        n_sub = max(1, -(-len(ref) * 8 // 1024))
        assert tab[u + 1, 1] - tab[u, 1] == n_sub
    assert desc.nsub == tab[-1, 1]
    assert (desc.width, desc.height, desc.bpm, desc.mcus_x, desc.mcus_y) == (72, 40, 6, 5, 3)
    assert desc.total_blocks == J['total_blocks']
    assert p.pack_seconds >= 0 and p.compressed_bytes == len(d)


def _reason(lib, data):
    from rmem_ocu_amd import _lib
    info = _lib.JpegInfo()
    rc = lib.rmem_jpeg_parse(data, len(data), ctypes.byref(info))
    return rc, lib.rmem_last_error_string().decode()


def test_rejects_progressive_cmyk_truncated(lib):
    from rmem_ocu_amd import jpeg
    from rmem_ocu_amd._lib import RmemError
    a = image(24, 40, 5)
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', progressive=True)
    prog = b.getvalue()
    rc, why = _reason(lib, prog)
    assert rc != 0 and 'progressive' in why
    b = io.BytesIO()
    Image.fromarray(a).convert('CMYK').save(b, 'JPEG')
    rc, why = _reason(lib, b.getvalue())
    assert rc != 0 and 'CMYK' in why
    d = encode(a, '420')
    rc, why = _reason(lib, d[:len(d) // 2])
    assert rc != 0 and 'truncated' in why
    rc, why = _reason(lib, d[:100])
    assert rc != 0 and 'truncated' in why
    with pytest.raises(RmemError, match='progressive'):
        jpeg.JpegClip([prog])
    with pytest.raises(RmemError, match='one size'):
        jpeg.JpegClip([encode(image(16, 16), '420'), encode(image(16, 24), '420')])
    i = d.index(b'\xff\xc0')
    assert d[i + 11] == 0x22                  # first component of SOF0: h2v2
    h4v1 = d[:i + 11] + b'\x41' + d[i + 12:]   # 4:1:1
    with pytest.raises(RmemError, match='sampling'):
        jpeg.parse(h4v1)


def test_rejects_twelve_bit_and_arithmetic(lib):
    d = bytearray(encode(image(16, 16), '444'))
    i = d.index(b'\xff\xc0')
    twelve = bytes(d[:i + 4]) + b'\x0c' + bytes(d[i + 5:])
    rc, why = _reason(lib, twelve)
    assert rc != 0 and '12-bit' in why
    arith = bytes(d[:i + 1]) + b'\xc9' + bytes(d[i + 2:])
    rc, why = _reason(lib, arith)
    assert rc != 0 and 'arithmetic' in why


@pytest.mark.parametrize('mode', ['L', '444', '422', '420'])
@pytest.mark.parametrize('hw', [(1, 1), (7, 9), (17, 33), (64, 96)])
@pytest.mark.parametrize('quality', [50, 90, 100])
def test_restatement_matches_pillow_bit_for_bit(mode, hw, quality):
    a = image(*hw, seed=hw[0] * 7 + quality)
    for kw in ({}, {'optimize': True}, {'restart_marker_blocks': 2}):
        d = encode(a, mode, quality, **kw)
        ref = np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        assert np.array_equal(jpeg_ref.decode(d), ref), (mode, hw, quality, kw)
