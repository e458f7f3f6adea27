"""Palette-PNG output, host side (no GPU): the Python restatement of the stream format (tests/png_ref.py) against zlib and Pillow,
rmem_ocu_amd.png.wrap against Pillow, rmem_png_zlib_bound / rmem_png_workspace_bytes, the argument checks of
rmem_png_encode_labels, and the un-squeeze table against save_mask's loop."""
import functools
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref as P


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def reference(name):
    return P.zlib_stream(P.case(name))


def decodes_to(data, lab, palette):
    im = Image.open(io.BytesIO(data))
    im.load()                                           # Pillow checks every chunk's CRC-32, zlib the Adler-32
    return im.mode == 'P' and im.size == (lab.shape[1], lab.shape[0]) and np.array_equal(np.array(im), lab) and im.getpalette() == palette


@pytest.mark.parametrize('name', P.case_names())
def test_restatement_against_zlib_and_pillow(name):
    from rmem_ocu_amd.evaluator import _davis_palette
    lab = P.case(name)
    H, W = lab.shape
    stream = reference(name)
    assert stream[:2] == b'\x78\x01'
    assert zlib.decompress(stream) == P.filtered(lab).tobytes()
    assert 0 < len(stream) <= P.zlib_bound(H, W)
    assert P.davis_palette() == _davis_palette()
    assert decodes_to(P.wrap(stream, H, W), lab, _davis_palette())


def test_run_tokens_at_the_edges():
    """L - 1 = 0, 1, 2 -> literals only; 3 -> the shortest match; 258 + (0, 1, 2, 3); two matches of 258"""
    lit, m = ('lit', 7), lambda t: ('match', t)
    assert P.run_tokens(7, 1) == [lit] and P.run_tokens(7, 2) == [lit, lit] and P.run_tokens(7, 3) == [lit, lit, lit]
    assert P.run_tokens(7, 4) == [lit, m(3)]
    assert P.run_tokens(7, 259) == [lit, m(258)] and P.run_tokens(7, 260) == [lit, m(258), lit]
    assert P.run_tokens(7, 261) == [lit, m(258), lit, lit] and P.run_tokens(7, 262) == [lit, m(258), m(3)]
    assert P.run_tokens(7, 517) == [lit, m(258), m(258)] and P.run_tokens(7, 518) == [lit, m(258), m(258), lit]
    assert P.length_code(258) == (285, 0, 0) and P.length_code(257) == (284, 5, 30) and P.length_code(3) == (257, 0, 0)
    assert P.length_code(10) == (264, 0, 0) and P.length_code(11) == (265, 1, 0) and P.length_code(114) == (279, 4, 15)
    assert P.length_code(115) == (280, 4, 0)


def test_value_2_merges_with_the_filter_byte():
    assert P.row_runs(P.filtered(P.case('run_v2_w63'))[0]) == [(2, 64)]
    assert P.row_runs(P.filtered(P.case('run_v1_w63'))[0]) == [(2, 1), (1, 63)]
    f = P.filtered(P.case('alternating_rows'))
    assert set(f[:, 1:].ravel().tolist()) == {0, 1, 255}


def test_wrap_around_zlib_compress():
    """png.wrap without the kernel: any valid zlib stream of the filtered bytes makes a file Pillow decodes to the labels"""
    from rmem_ocu_amd import png
    from rmem_ocu_amd.evaluator import _davis_palette
    for name in ('symbols_5x7', 'blobs_97x131', 'run_v1_w1'):
        lab = P.case(name)
        H, W = lab.shape
        data = png.wrap(zlib.compress(P.filtered(lab).tobytes()), H, W)
        assert decodes_to(data, lab, _davis_palette())
        assert data == P.wrap(zlib.compress(P.filtered(lab).tobytes()), H, W)
    grey = [v for i in range(256) for v in (i, i, i)]
    lab = P.case('symbols_5x7')
    assert decodes_to(png.wrap(reference('symbols_5x7'), 5, 7, palette=grey), lab, grey)
    from rmem_ocu_amd._lib import RmemError
    with pytest.raises(RmemError, match='palette'):
        png.wrap(b'', 5, 7, palette=[0, 0, 0])


def test_zlib_bound(lib):
    for name in P.case_names():
        H, W = P.case(name).shape if 'blobs_' not in name else tuple(int(v) for v in name[6:].split('x'))
        want = 2 + -(-(3 + 9 * (W + 1) * H + 7) // 8) + 4
        assert lib.rmem_png_zlib_bound(H, W) == want == P.zlib_bound(H, W)
    assert lib.rmem_png_zlib_bound(1, 1) == 10
    assert lib.rmem_png_zlib_bound(8192, 8192) == P.zlib_bound(8192, 8192)          # H * W = 2^26: the largest frame
    for bad in ((0, 5), (5, 0), (-1, 5), (8192, 8193)):
        assert lib.rmem_png_zlib_bound(*bad) == 0


def test_noise_stays_within_and_close_to_the_bound():
    """every filtered byte a 9-bit literal but each row's filter byte: the stream reaches the bound to within (H + 10) bits"""
    stream = reference('noise9_64x200')
    bound = P.zlib_bound(64, 200)
    print(f'noise9 64x200: {len(stream)} of {bound} bytes = {len(stream) / bound:.4f}; uniform noise: '
          f'{len(reference("noise_64x200")) / bound:.4f}')
    assert 0.98 * bound < len(stream) <= bound
    assert len(reference('noise_64x200')) <= bound


def test_workspace_bytes(lib):
    f = lib.rmem_png_workspace_bytes
    sizes = [f(n, 40, 50) for n in (1, 2, 3, 64, 65)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert f(1, 40, 50) >= 3 * 40 * 4 and f(2, 480, 854) < f(2, 481, 854)
    for bad in ((0, 40, 50), (1, 0, 50), (1, 40, 0), (1, 8192, 8193)):
        assert f(*bad) == 0


def test_encode_argument_checks_need_no_gpu(lib):
    call = lib.rmem_png_encode_labels
    for n, H, W in ((0, 40, 50), (1, 0, 50), (1, 40, -3)):
        assert call(16, n, H, W, None, 16, 16, 16, None) != 0
        assert b'positive' in lib.rmem_last_error_string()
    assert call(16, 1, 8192, 8193, None, 16, 16, 16, None) != 0
    assert b'2^26' in lib.rmem_last_error_string()
    for args in ((None, 1, 40, 50, None, 16, 16, 16, None), (16, 1, 40, 50, None, None, 16, 16, None),
                 (16, 1, 40, 50, None, 16, None, 16, None), (16, 1, 40, 50, None, 16, 16, None, None)):
        assert call(*args) != 0
        assert b'null' in lib.rmem_last_error_string()


def test_squeeze_table_equals_save_masks_loop():
    from rmem_ocu_amd import png
    for squeeze_idx in ([0, 4, 9], [0], [0, 255, 1, 1, 7], list(range(40))):
        lut = png.squeeze_lut(squeeze_idx)
        assert lut.dtype == np.uint8 and lut.shape == (256,)
        assert np.array_equal(lut, P.squeeze_lut(squeeze_idx))
    assert png.squeeze_lut([0, 4, 9]).tolist() == [0, 4, 9] + [0] * 253


def test_save_mask_agrees_with_the_table(tmp_path):
    """save_mask itself (Pillow) on all 256 values against the table"""
    from rmem_ocu_amd import evaluator, png
    mask = np.arange(256, dtype=np.uint8).reshape(16, 16)
    path = str(tmp_path / 'm.png')
    evaluator.save_mask(mask, path, squeeze_idx=[0, 4, 9])
    assert np.array_equal(np.array(Image.open(path)), png.squeeze_lut([0, 4, 9])[mask])


def test_host_tensors_and_bad_stacks_are_refused():
    import torch
    from rmem_ocu_amd import evaluator, png
    from rmem_ocu_amd._lib import RmemError
    x = torch.zeros(3, 8, 8, dtype=torch.uint8)
    for fn in (png.encode_zlib, png.encode_label_stack):
        with pytest.raises(RmemError, match='device'):
            fn(x)
    with pytest.raises(RmemError, match='device'):
        evaluator.save_masks(x, ['a', 'b', 'c'])
