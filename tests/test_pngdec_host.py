"""Palette-PNG input, host side (no GPU): the Python restatement (tests/pnginf_ref.py) against zlib and Pillow, the case table's own
claims, rmem_ocu_amd.png.parse / PackedPngs, rmem_png_decode_workspace_bytes, the argument checks of rmem_png_decode_labels and
of the Python entry points."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import pnginf_ref as R


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize('name', R.case_names())
def test_restatement_against_zlib_and_pillow(name):
    c = R.cases()[name]
    _, stream = R.split_png(c.png)
    raw, _ = R.inflate(stream)
    assert raw == zlib.decompress(stream)
    got = R.decode_png(c.png)
    assert np.array_equal(got, np.array(Image.open(io.BytesIO(c.png))))
    assert np.array_equal(got, c.label)


def test_cases_exercise_what_they_claim():
    R.assert_cases_exercise_what_they_claim()
    assert len({c.label.shape for c in R.cases().values()}) >= 15


def test_filters_and_packing_round_trip():
    rows = R.noise(9, 33, 256, 4)
    for filters in ([k] * 9 for k in range(5)):
        filt = R.filter_rows(rows, filters)
        assert filt[:, 0].tolist() == filters and np.array_equal(R.unfilter_rows(filt), rows)
    for depth in (1, 2, 4):
        lab = R.noise(3, 13, 1 << depth, depth)
        assert np.array_equal(R.unpack_rows(R.pack_rows(lab, depth), depth, 13), lab)
    assert R.pack_rows(np.array([[1, 0, 1]]), 1).tolist() == [[0b10111111]]           # most significant bit first, padding set


def test_corrupt_streams_are_refused_by_the_restatement_and_by_pillow():
    for name, (data, bit) in R.corrupt_cases().items():
        assert bit in (R.ST_INPUT, R.ST_SIZE, R.ST_RANGE, R.ST_CODE, R.ST_HEADER, R.ST_ADLER, R.ST_FILTER), name
        with pytest.raises((ValueError, AssertionError)):
            R.decode_png(data)
        if name != 'one_match_too_many':            # Pillow stops at the frame's last byte and never sees the extra match
            with pytest.raises(OSError):
                Image.open(io.BytesIO(data)).load()


def test_parse_fields():
    from rmem_ocu_amd import png
    c = R.cases()['pillow_bits4_97x131']
    info = png.parse(c.png)
    assert (info.width, info.height, info.bit_depth, info.colour_type, info.interlace) == (131, 97, 4, 3, 0)
    assert info.palette is not None and len(info.palette) % 3 == 0
    assert b''.join(c.png[a:b] for a, b in info.idat_ranges) == R.split_png(c.png)[1]
    g = png.parse(R.cases()['grey_40x50'].png)
    assert (g.width, g.height, g.bit_depth, g.colour_type, g.palette) == (50, 40, 8, 0, None)


@pytest.mark.parametrize('split', (1, 7, 4096))
def test_parse_reassembles_multiple_idat_chunks(split):
    from rmem_ocu_amd import png
    lab = R.noise(64, 200, 256, 7)
    stream = R.compress(R.filtered_bytes(lab), 'dynamic')
    data = R.png_around(stream, 64, 200, idat_split=split)
    info = png.parse(data)
    assert len(info.idat_ranges) == -(-len(stream) // split) and len(stream) > 4096
    assert b''.join(data[a:b] for a, b in info.idat_ranges) == stream


def test_parse_refuses_by_name():
    from rmem_ocu_amd import png
    from rmem_ocu_amd._lib import RmemError
    stream = zlib.compress(bytes(100))
    ok = R.png_around(stream, 4, 4)
    for kw, why in ((dict(interlace=1), 'interlaced'), (dict(depth=16, colour_type=0), '16-bit'), (dict(colour_type=2), 'colour type 2'),
                    (dict(colour_type=4), 'colour type 4'), (dict(colour_type=6), 'colour type 6'), (dict(depth=4, colour_type=0), 'grey at bit depth 4')):
        data = R.png_around(stream, 4, 4, **{'depth': 8, 'colour_type': 3, **kw})
        with pytest.raises(png.PngUnsupported, match=why):
            png.parse(data)
        assert png.parse(data, check=False).width == 4                      # a sound file: only the format is refused
    with pytest.raises(png.PngUnsupported, match='2\\^26'):
        png.parse(R.png_around(stream, 8192, 8193))
    with pytest.raises(RmemError, match='signature') as e:
        png.parse(b'\x89PNX' + ok[4:])
    assert not isinstance(e.value, png.PngUnsupported)
    ihdr_end = 8 + 25
    with pytest.raises(RmemError, match='missing IHDR'):
        png.parse(ok[:8] + ok[ihdr_end:])
    idat_at = ok.index(b'IDAT') - 4
    iend_at = ok.index(b'IEND') - 4
    with pytest.raises(RmemError, match='missing IDAT'):
        png.parse(ok[:idat_at] + ok[iend_at:])
    with pytest.raises(RmemError, match='missing IEND'):
        png.parse(ok[:iend_at])
    for at in (ihdr_end - 6, idat_at + 10, len(ok) - 2):                    # a byte of IHDR's body, of IDAT's body, of IEND's CRC
        bad = bytearray(ok)
        bad[at] ^= 0x40
        with pytest.raises(RmemError, match='CRC'):
            png.parse(bytes(bad))


def test_packed_pngs_layout():
    from rmem_ocu_amd import png
    from rmem_ocu_amd._lib import PngDesc, RmemError
    names = R.by_size()[(64, 200)]
    files = [R.cases()[n].png for n in names]
    pk = png.PackedPngs(files)
    assert len(pk) == len(files) and tuple(pk.shape) == (len(files), 64, 200) and pk.buf.dtype.is_floating_point is False
    buf = pk.buf.numpy()
    assert struct.calcsize('qqii') == 24 == len(bytes(pk.descs)) // len(files) and PngDesc.bit_depth.offset == 16
    end = 0
    for d, f in zip(pk.descs, files):
        stream = R.split_png(f)[1]
        assert d.offset % 8 == 0 and d.offset >= end and d.bytes == len(stream) and (d.bit_depth, d.colour_type) == (8, 3)
        assert buf[d.offset:d.offset + d.bytes].tobytes() == stream
        end = d.offset + d.bytes + 8
        assert not buf[d.offset + d.bytes:end].any() and end <= buf.size      # at least 8 zero bytes behind every stream
    assert pk.compressed_bytes == sum(d.bytes for d in pk.descs)
    mixed = png.PackedPngs([R.cases()[n].png for n in R.by_size()[(3, 13)]])
    assert sorted(d.bit_depth for d in mixed.descs) == [1, 2, 4]
    with pytest.raises(RmemError, match='share one size'):
        png.PackedPngs([files[0], R.cases()['edge_5x7'].png])
    with pytest.raises(RmemError, match='no files'):
        png.PackedPngs([])


def test_paths_and_bytes(tmp_path):
    from rmem_ocu_amd import png
    c = R.cases()['edge_5x7']
    p = tmp_path / 'a.png'
    p.write_bytes(c.png)
    a, b = png.PackedPngs([str(p)]), png.PackedPngs([c.png])
    assert a.buf.numpy().tobytes() == b.buf.numpy().tobytes() and bytes(a.descs) == bytes(b.descs)


def test_decode_workspace_bytes(lib):
    f = lib.rmem_png_decode_workspace_bytes
    sizes = [f(n, 40, 50) for n in (1, 2, 3, 64, 65)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert f(2, 480, 854) < f(2, 481, 854) and f(2, 480, 854) < f(2, 480, 870)
    for n, H, W in ((1, 1, 1), (3, 40, 50), (64, 480, 854), (1, 8192, 8192)):
        assert f(n, H, W) >= n * H * (1 + W)                                 # the filtered bytes at depth 8
    for bad in ((0, 40, 50), (1, 0, 50), (1, 40, 0), (1, 8192, 8193), (-1, 4, 4)):
        assert f(*bad) == 0


def test_decode_argument_checks_need_no_gpu(lib):
    call = lib.rmem_png_decode_labels
    for n, H, W in ((0, 40, 50), (1, 0, 50), (1, 40, -3)):
        assert call(16, 16, n, H, W, None, 16, 16, 16, None) != 0
        assert b'positive' in lib.rmem_last_error_string()
    assert call(16, 16, 1, 8192, 8193, None, 16, 16, 16, None) != 0
    assert b'2^26' in lib.rmem_last_error_string()
    for args in ((None, 16, 1, 40, 50, None, 16, 16, 16, None), (16, None, 1, 40, 50, None, 16, 16, 16, None),
                 (16, 16, 1, 40, 50, None, None, 16, 16, None), (16, 16, 1, 40, 50, None, 16, None, 16, None),
                 (16, 16, 1, 40, 50, None, 16, 16, None, None)):
        assert call(*args) != 0
        assert b'null' in lib.rmem_last_error_string()
    assert call(12, 16, 1, 40, 50, None, 16, 16, 16, None) != 0
    assert b'aligned' in lib.rmem_last_error_string()


def test_status_bits_mirror_the_header():
    from conftest import ROOT
    from rmem_ocu_amd import png
    text = open(os.path.join(ROOT, 'include', 'rmem.h')).read()
    for name in ('INPUT', 'SIZE', 'RANGE', 'CODE', 'HEADER', 'ADLER', 'FILTER', 'DESC'):
        assert f'#define RMEM_PNG_ST_{name} {getattr(png, "ST_" + name)}\n' in text
        assert getattr(png, 'ST_' + name) == getattr(R, 'ST_' + name) and getattr(png, 'ST_' + name) in png.STATUS_NAMES


def test_host_tensors_and_bad_luts_are_refused():
    import torch
    from rmem_ocu_amd import evaluator, png
    from rmem_ocu_amd._lib import RmemError
    c = R.cases()['edge_5x7']
    pk = png.PackedPngs([c.png])
    with pytest.raises(RmemError, match='device'):
        png.decode_labels_into(pk, torch.zeros(1, 5, 7, dtype=torch.uint8), 0, 1)
    with pytest.raises(RmemError, match='device'):
        png.decode_label_stack([c.png], 'cpu')
    with pytest.raises(RmemError, match='device'):
        evaluator.labels_from_pngs([c.png], torch.device('cpu'))
    for lut in (np.zeros(255, np.uint8), np.zeros(256, np.int32), np.zeros((2, 256), np.uint8)):
        with pytest.raises(RmemError, match='lut'):
            png._device_lut(lut, torch.device('cpu'), 'test')
    for lut in (torch.zeros(255, dtype=torch.uint8), torch.zeros(512, dtype=torch.uint8)[::2], torch.zeros(256, dtype=torch.int32)):
        with pytest.raises(RmemError, match='lut'):
            png._device_lut(lut, torch.device('cpu'), 'test')
