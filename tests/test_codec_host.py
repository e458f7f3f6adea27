"""Host plumbing of the image codecs (rmem_ocu_amd._codec): the check of the offsets a device call wrote, and the palette.  No GPU."""
import pytest

import png_ref as P


def test_split_files():
    from rmem_ocu_amd import _codec
    from rmem_ocu_amd._lib import RmemError
    assert _codec.split_files(b'abcdefg', [0, 3, 7], 7, 'png.test') == [b'abc', b'defg']
    with pytest.raises(RmemError, match='png.test'):
        _codec.split_files(b'abcdefg', [1, 3, 7], 7, 'png.test')            # does not start at 0
    for off in ([0, 3, 3], [0, 4, 3]):                                      # not strictly increasing
        with pytest.raises(RmemError, match='jpeg.test'):
            _codec.split_files(b'abcdefg', off, 7, 'jpeg.test')
    with pytest.raises(RmemError, match='png.test'):
        _codec.split_files(b'abcdefg', [0, 3, 7], 6, 'png.test')            # more bytes than the buffer holds


def test_one_palette():
    from rmem_ocu_amd import _codec, evaluator
    assert _codec.davis_palette() == P.davis_palette()
    assert evaluator._davis_palette is _codec.davis_palette
