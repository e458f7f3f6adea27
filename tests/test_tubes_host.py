"""The label tubes without a GPU: the two restatements of the contract (tubes_ref: scipy.ndimage.label on the 3-D structures, and a
plain union-find over pieces) against each other on every content, frames written out by hand, what the contents claim, the seven
new symbols, the workspace query, and every refusal of the entry points and of the Python functions."""
import os
import re

import numpy as np
import pytest

import components_ref as C
import tubes_ref as R
from conftest import ROOT

CONFIGS = [(4, 1), (4, 9), (8, 1), (8, 9)]
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 33, 65), (2, 32, 64), (3, 5, 7), (5, 31, 127)]


@pytest.mark.parametrize('name', R.CONTENTS)
def test_the_two_restatements_agree(name):
    for shape in SHAPES:
        a = R.content(name, *shape)
        for conn, temp in CONFIGS:
            assert np.array_equal(R.tubes(a, conn, temp), R.tubes_by_pieces(a, conn, temp)), (name, shape, conn, temp)


def _all(a, conn=8, temp=1):
    return R.everything(np.asarray(a, dtype=np.uint8), conn, temp)


def _of_value(ref, v):
    return ref['table'][ref['table'][:, 1] == v]


@pytest.mark.parametrize('conn,temp', CONFIGS)
def test_bar_that_splits_and_merges(conn, temp):
    a = np.zeros((4, 3, 8), dtype=np.uint8)
    for f in range(4):
        a[f, 1, 1:7] = R.BAR[f]
    ref = _all(a, conn, temp)
    rows = _of_value(ref, 1)
    assert len(rows) == 1 and rows[0].tolist() == [1 * 8 + 1, 1, 6 + 4 + 4 + 6, 6, 0, 3, 0, 0, 0, 6]
    E = ref['events']
    assert E[0, 1].tolist() == [0, 0, 1, 0] and E[3, 1].tolist() == [0, 0, 0, 1]
    assert E[:, :, 0].sum() == 0 and E[:, :, 1].sum() == 0 and E[:, :, 2].sum() == 1 and E[:, :, 3].sum() == 1
    assert ref['links'][0, 9].tolist() == [24, -1, 9, 13] and ref['links'][3, 9].tolist() == [9, 13, 24, -1]
    assert ref['links'][1, 13].tolist() == [9, 9, 13, 13] and ref['links'][1, 10].tolist() == [24, -1, 24, -1]


def _speck(frames, n=6):
    a = np.zeros((n, 6, 6), dtype=np.uint8)
    a[frames[0]:frames[1] + 1, 2:4, 2:4] = 5
    return a


def test_speck_on_the_background():
    a = _speck((2, 3))
    assert not R.clean(a, 3, 0).any()
    assert np.array_equal(R.clean(a, 2, 0), a) and np.array_equal(R.clean(a, 0, 0), a) and np.array_equal(R.clean(a, 1, 0), a)
    for frames in ((0, 1), (4, 5)):                                 # not closed: frame 0 is given, the last frame's tube goes on
        a = _speck(frames)
        assert np.array_equal(R.clean(a, 3, 0), a) and np.array_equal(R.clean(a, 7, 6), a)


def test_speck_inside_an_object_becomes_the_object():
    a = np.zeros((6, 6, 6), dtype=np.uint8)
    a[:, 1:5, 1:5] = 1
    a[2:4, 2, 2] = 2
    want = a.copy()
    want[2:4, 2, 2] = 1
    assert np.array_equal(R.clean(a, 3, 0), want) and np.array_equal(R.clean(a, 2, 0), a)
    a[2:4, 1, 1] = 2                                                # a second piece of the speck at the object's corner: it sees 0 and 1
    want = a.copy()
    want[2:4, 2, 2] = 1
    want[2:4, 1, 1] = 0
    assert np.array_equal(R.clean(a, 3, 0, connectivity=4), want)


def test_line_that_moves_one_column_per_frame():
    n = 5
    a = np.zeros((n, 4, 7), dtype=np.uint8)
    for f in range(n):
        a[f, :, f] = 1
    for conn in (4, 8):
        assert len(_of_value(_all(a, conn, 1), 1)) == n
        rows = _of_value(_all(a, conn, 9), 1)
        assert len(rows) == 1 and rows[0].tolist() == [0, 1, 4 * n, n, 0, n - 1, 0, 0, 1, 4]


def _gap(kind):
    a = np.zeros((6, 6, 6), dtype=np.uint8)
    if kind == 'inside':
        a[:, 1:5, 1:5] = 1
        a[2:4, 2, 2] = 0
    elif kind == 'edge':
        a[:, 0:5, 1:5] = 1
        a[2:4, 0, 2] = 0
    else:                                                           # between two objects
        a[:, 1:5, 1:3] = 1
        a[:, 1:5, 3:5] = 2
        a[2:4, 2, 2] = 0
    return a


def test_gap_in_time():
    a = _gap('inside')
    filled = a.copy()
    filled[2:4, 2, 2] = 1
    assert np.array_equal(R.clean(a, 0, 2), filled) and np.array_equal(R.clean(a, 0, 1), a) and np.array_equal(R.clean(a, 9, 0), a)
    for kind in ('edge', 'between'):
        a = _gap(kind)
        assert np.array_equal(R.clean(a, 0, 2), a) and np.array_equal(R.clean(a, 0, 6), a), kind


def test_one_frame():
    a = R.content('drift', 1, 33, 65)
    for conn, temp in CONFIGS:
        ref = _all(a, conn, temp)
        assert np.array_equal(ref['tubes'], C.roots(a, conn)) and not ref['events'].any()
        assert (ref['links'] == np.array([33 * 65, -1, 33 * 65, -1])).all()
        assert np.array_equal(R.clean(a, 5, 5, conn, temp), a)


def test_contents_are_what_they_claim():
    n, H, W = shape = (5, 31, 127)
    assert _all(R.content('noise', *shape), 4, 1)['total'] > n * H * W // 8
    drift = _all(R.content('drift', *shape), 8, 1)['table']
    assert ((drift[:, 1] != 0) & (drift[:, 4] == 0) & (drift[:, 5] == n - 1)).any()
    assert ((drift[:, 1] != 0) & (drift[:, 5] - drift[:, 4] == 1)).any(), 'a 2-frame speck'
    bars = _all(R.content('bars', *shape), 8, 1)['events']
    assert bars[:, 1, 2].sum() > 0 and bars[:, 1, 3].sum() > 0
    checker = _all(R.content('checker', *shape), 4, 1)
    assert checker['total'] == H * W and (checker['table'][:, 3] == n).all() and (checker['table'][:, 2] == n).all()
    assert _all(R.content('checker', *shape), 8, 1)['total'] == 2
    assert _all(R.content('flip', *shape), 4, 1)['total'] == n * H * W
    stairs = _of_value(_all(R.content('stairs', 6, 97, 131), 8, 1), 1)
    assert len(stairs) == 1 and stairs[0, 3] == 6 and stairs[0, 4] == 0 and stairs[0, 5] == 5


# ------------------------------------------------------------------------------------------------------------------ the library
NEW = ('rmem_label_tubes_workspace_bytes', 'rmem_label_tubes', 'rmem_label_tube_lineage', 'rmem_label_tube_events', 'rmem_label_tube_index',
       'rmem_label_tube_table', 'rmem_label_tube_clean')


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from rmem_ocu_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rmem.h')).read(), flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/rmem.h'
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rmem_abi_version() == 15


def test_workspace_bytes(lib):
    ws = lib.rmem_label_tubes_workspace_bytes
    assert ws(2, 3, 5) == 2 * 3 * 5 * (4 + 16 + 4 + 4) == 840       # roots, stats, tubes, rank
    assert ws(1, 1, 1) == 28 and ws(64, 480, 854) == 64 * 480 * 854 * 28
    assert ws(31, 8192, 8192) == 31 * (1 << 26) * 28 and ws(32, 8192, 8192) == 0      # n * H * W = 2^31
    assert ws(2047, 1024, 1024) == 2047 * (1 << 20) * 28 and ws(2048, 1024, 1024) == 0
    for n, H, W in ((1, 8193, 8192), (1, 1, (1 << 26) + 1), (0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, -1), (65535, 8192, 8192)):
        assert ws(n, H, W) == 0, (n, H, W)


def test_entry_points_refuse_on_the_host(lib):
    """non-zero, a message that names the entry point, nothing launched (there is no GPU in this tier)"""
    fake = 4096                                                     # a non-null address that is never dereferenced on the host
    geometry = (((0, 4, 4), b'1..65535'), ((65536, 4, 4), b'1..65535'), ((1, 0, 4), b'positive'), ((1, 4, -1), b'positive'),
                ((1, 8193, 8193), b'2^26'), ((32, 8192, 8192), b'2^31 - 1'))
    # name -> (arguments, positions of the pointers, position of n)
    entries = {
        'rmem_label_tubes': ([fake, fake, 2, 4, 4, 1, fake, fake, None], (0, 1, 6, 7), 2),
        'rmem_label_tube_lineage': ([fake, fake, 2, 4, 4, 9, fake, None], (0, 1, 6), 2),
        'rmem_label_tube_events': ([fake, fake, fake, 2, 4, 4, fake, None], (0, 1, 2, 6), 3),
        'rmem_label_tube_index': ([fake, 2, 4, 4, fake, fake, None], (0, 4, 5), 1),
        'rmem_label_tube_table': ([fake, fake, fake, fake, fake, 2, 4, 4, 3, fake, None], (0, 1, 2, 3, 4, 9), 5),
        'rmem_label_tube_clean': ([fake, fake, fake, fake, fake, fake, fake, 2, 4, 4, 3, 0, None], (0, 1, 2, 3, 4, 5, 6), 7),
    }
    cases = []
    for name, (args, pointers, at) in entries.items():
        for k in pointers:
            bad = list(args)
            bad[k] = None
            cases.append((name, bad, b'null'))
        for (n, H, W), word in geometry:
            bad = list(args)
            bad[at:at + 3] = [n, H, W]
            cases.append((name, bad, word))
    for name in ('rmem_label_tubes', 'rmem_label_tube_lineage'):
        for temporal in (0, 2, 8, -1, 27):
            bad = list(entries[name][0])
            bad[5] = temporal
            cases.append((name, bad, b'temporal must be 1 or 9'))
    bad = list(entries['rmem_label_tube_table'][0])
    bad[8] = -1
    cases.append(('rmem_label_tube_table', bad, b'rows must not be negative'))
    for k in (10, 11):
        bad = list(entries['rmem_label_tube_clean'][0])
        bad[k] = -1
        cases.append(('rmem_label_tube_clean', bad, b'negative'))
    for name, args, word in cases:
        rc = getattr(lib, name)(*args)
        msg = lib.rmem_last_error_string()
        assert rc != 0 and name.encode() + b':' in msg and word in msg, (name, args, msg)


def test_python_refusals():
    import torch
    from rmem_ocu_amd import tubes
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import object_events, object_tracks, remove_flicker
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    stack_calls = (tubes.label_tubes, tubes.lineage, tubes.piece_events, tubes.tube_table, tubes.clean_tubes, remove_flicker,
                   lambda t, *a, **k: object_events(t, 3, *a, **k), lambda t, *a, **k: object_tracks(t, 3, *a, **k))
    for call in stack_calls:
        for bad in (x, x.int(), None):                              # a host tensor, the wrong dtype, no tensor
            with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
                call(bad)
        for bad in (6, 0, 4.0, None, True):
            with pytest.raises(RmemError, match=r'connectivity must be 4 or 8 \(got'):
                call(x, connectivity=bad)
        for bad in (0, 3, 27, 9.0, None, True):
            with pytest.raises(RmemError, match=r'temporal must be 1 or 9 \(got'):
                call(x, temporal=bad)
    for bad in (-1, 2.5, None):
        with pytest.raises(RmemError, match=r'tubes.clean_tubes: min_frames must be a non-negative integer \(got'):
            tubes.clean_tubes(x, min_frames=bad)
        with pytest.raises(RmemError, match=r'tubes.clean_tubes: max_hole_frames must be a non-negative integer \(got'):
            tubes.clean_tubes(x, max_hole_frames=bad)
        with pytest.raises(RmemError, match='min_frames'):
            remove_flicker(x, min_frames=bad)
        with pytest.raises(RmemError, match='max_hole_frames'):
            remove_flicker(x, fill_frames=bad)
    for out in (x[:1], x[0], torch.zeros(2, 4, 5, dtype=torch.uint8), np.zeros((2, 4, 4), dtype=np.uint8)):
        with pytest.raises(RmemError, match='out must be a tensor of the labels\' shape'):
            tubes.clean_tubes(x, out=out)
    for bad in (0, 256, None, 2.5):
        with pytest.raises(RmemError, match=r'evaluator.object_events: num_objs must be an integer in 1\.\.255 \(got'):
            object_events(x, bad)
        with pytest.raises(RmemError, match=r'evaluator.object_tracks: num_objs must be an integer in 1\.\.255 \(got'):
            object_tracks(x, bad)


def test_package_does_not_import_scipy_or_the_oracle():
    src = open(os.path.join(ROOT, 'rmem_ocu_amd', 'tubes.py')).read()
    assert 'scipy' not in src and 'oracle' not in src and 'ref_cpu' not in src
