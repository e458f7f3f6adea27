"""The connected components without a GPU: the scipy restatement (components_ref) against 5 x 7 maps whose roots, statistics and
cleaned output are written out by hand, the five new symbols, the tile and workspace queries, and every refusal of the three
entry points and of the Python functions."""
import ctypes
import os
import re

import numpy as np
import pytest

import components_ref as R
from conftest import ROOT

ABSENT = (0, 256, -1, 0)


def _check(frame, connectivity, roots, at_roots, table):
    """roots as a whole map, stats as {root: entry} with every other entry absent, table as {value: entry} with the rest absent"""
    frame = np.array(frame, dtype=np.uint8)[None]
    r = R.roots(frame, connectivity)
    assert r.dtype == np.int32 and r[0].tolist() == roots
    S, T = R.stats(frame, connectivity)
    assert S.dtype == np.int32 and S.shape == (1, 35, 4) and T.dtype == np.int32 and T.shape == (1, 256, 3)
    for p in range(35):
        assert tuple(S[0, p]) == at_roots.get(p, ABSENT), p
    for v in range(256):
        assert tuple(T[0, v]) == table.get(v, (0, 0, -1)), v
    return frame


def _clean(frame, connectivity, rule, want):
    assert R.clean(frame, *rule, connectivity=connectivity)[0].tolist() == want, rule


A = [[0, 0, 0, 0, 0, 0, 0],
     [0, 1, 1, 1, 0, 0, 0],
     [0, 1, 0, 1, 0, 2, 0],
     [0, 1, 1, 1, 0, 0, 0],
     [0, 0, 0, 0, 0, 0, 0]]


@pytest.mark.parametrize('connectivity', [4, 8])
def test_hole_in_one_object_and_speck_on_the_background(connectivity):
    roots = [[0, 0, 0, 0, 0, 0, 0],
             [0, 8, 8, 8, 0, 0, 0],
             [0, 8, 16, 8, 0, 19, 0],
             [0, 8, 8, 8, 0, 0, 0],
             [0, 0, 0, 0, 0, 0, 0]]
    frame = _check(A, connectivity, roots, {0: (25, 1, 2, 1), 8: (8, 0, 0, 0), 16: (1, 1, 1, 0), 19: (1, 0, 0, 0)},
                   {0: (2, 25, 0), 1: (1, 8, 8), 2: (1, 1, 19)})
    filled = [row[:] for row in A]
    filled[2][2] = 1
    swept = [row[:] for row in A]
    swept[2][5] = 0
    both = [row[:] for row in filled]
    both[2][5] = 0
    _clean(frame, connectivity, (0, 0, False), A)                   # the identity
    _clean(frame, connectivity, (1, 0, False), filled)
    _clean(frame, connectivity, (0, 1, False), swept)
    _clean(frame, connectivity, (1, 1, False), both)
    _clean(frame, connectivity, (0, 0, True), A)                    # every object is one piece
    # everything goes: the hole is filled from the INPUT's components, the object around it falls to the background
    gone = [[0] * 7 for _ in range(5)]
    gone[2][2] = 1
    _clean(frame, connectivity, (35, 35, True), gone)


B = [[1, 1, 1, 2, 2, 2, 0],
     [1, 1, 0, 0, 2, 2, 0],
     [1, 1, 1, 2, 2, 2, 0],
     [3, 3, 3, 3, 3, 3, 0],
     [3, 0, 3, 3, 3, 3, 0]]


def test_holes_that_are_left_alone():
    """a hole between two objects (neighbours 1 and 2) and a hole that touches the border (row H - 1)"""
    roots = [[0, 0, 0, 3, 3, 3, 6],
             [0, 0, 9, 9, 3, 3, 6],
             [0, 0, 0, 3, 3, 3, 6],
             [21, 21, 21, 21, 21, 21, 6],
             [21, 29, 21, 21, 21, 21, 6]]
    frame = _check(B, 8, roots, {0: (8, 0, 3, 1), 3: (8, 0, 3, 1), 6: (5, 2, 3, 1), 9: (2, 1, 2, 0), 21: (11, 0, 2, 1), 29: (1, 3, 3, 1)},
                   {0: (3, 5, 6), 1: (1, 8, 0), 2: (1, 8, 3), 3: (1, 11, 21)})
    for rule in ((35, 0, False), (35, 0, True), (2, 0, False)):
        _clean(frame, 8, rule, B)
    # under 4 the objects do not see the hole's far end: 1 touches (1, 2) only, 2 touches (1, 3) only -- the hole still sees both
    S, _ = R.stats(frame, 4)
    assert tuple(S[0, 9]) == (2, 1, 2, 0) and tuple(S[0, 0]) == (8, 0, 3, 1)
    _clean(frame, 4, (35, 0, False), B)


C = [[1, 1, 1, 1, 1, 0, 0],
     [1, 2, 1, 1, 0, 3, 0],
     [1, 1, 1, 0, 3, 0, 0],
     [0, 0, 0, 0, 0, 0, 0],
     [4, 4, 0, 0, 0, 4, 4]]


def test_speck_inside_an_object_diagonal_link_and_tie_under_8():
    roots = [[0, 0, 0, 0, 0, 5, 5],
             [0, 8, 0, 0, 5, 12, 5],
             [0, 0, 0, 5, 12, 5, 5],
             [5, 5, 5, 5, 5, 5, 5],
             [28, 28, 5, 5, 5, 33, 33]]
    frame = _check(C, 8, roots, {0: (11, 0, 3, 1), 5: (17, 1, 4, 1), 8: (1, 1, 1, 0), 12: (2, 0, 1, 0), 28: (2, 0, 0, 1), 33: (2, 0, 0, 1)},
                   {0: (1, 17, 5), 1: (1, 11, 0), 2: (1, 1, 8), 3: (1, 2, 12), 4: (2, 2, 28)})
    inside = [row[:] for row in C]
    inside[1][1] = 1                                                # the speck of 2 lies wholly inside object 1: it becomes 1
    _clean(frame, 8, (0, 1, False), inside)
    largest = [row[:] for row in C]
    largest[4][5] = largest[4][6] = 0                               # two pieces of 4 with area 2: the smaller root stays
    _clean(frame, 8, (0, 0, True), largest)
    straddle = [row[:] for row in inside]
    straddle[1][5] = straddle[2][4] = 0                             # the piece of 3 touches 0 and 1: background
    straddle[4] = [0] * 7
    _clean(frame, 8, (0, 2, False), straddle)


def test_the_diagonal_link_is_cut_under_4():
    roots = [[0, 0, 0, 0, 0, 5, 5],
             [0, 8, 0, 0, 11, 12, 5],
             [0, 0, 0, 5, 18, 5, 5],
             [5, 5, 5, 5, 5, 5, 5],
             [28, 28, 5, 5, 5, 33, 33]]
    frame = _check(C, 4, roots, {0: (11, 0, 2, 1), 5: (16, 1, 4, 1), 8: (1, 1, 1, 0), 11: (1, 1, 3, 0), 12: (1, 0, 0, 0), 18: (1, 0, 0, 0),
                                 28: (2, 0, 0, 1), 33: (2, 0, 0, 1)},
                   {0: (2, 16, 5), 1: (1, 11, 0), 2: (1, 1, 8), 3: (2, 1, 12), 4: (2, 2, 28)})
    _clean(frame, 4, (1, 0, False), C)                              # the hole at (1, 4) lies between 1 and 3
    largest = [row[:] for row in C]
    largest[2][4] = 0                                               # a tie of two single pixels of 3: root 12 stays
    largest[4][5] = largest[4][6] = 0
    _clean(frame, 4, (0, 0, True), largest)


def test_whole_frame_component_and_frames_are_independent():
    stack = np.zeros((2, 5, 7), dtype=np.uint8)
    stack[1] = 7
    r = R.roots(stack, 8)
    S, T = R.stats(stack, 8)
    assert not r.any() and tuple(S[0, 0]) == (35, 256, -1, 1) and tuple(S[1, 0]) == (35, 256, -1, 1)
    assert tuple(T[0, 0]) == (1, 35, 0) and tuple(T[1, 7]) == (1, 35, 0) and tuple(T[1, 0]) == (0, 0, -1)
    assert np.array_equal(R.clean(stack, 35, 0, False), stack)      # a background that touches the border is no hole
    assert not R.clean(stack, 0, 35, False).any()                   # nb_min != nb_max: the whole frame of 7 falls to 0


# ------------------------------------------------------------------------------------------------------------------ the library
NEW = ('rmem_label_components_tile', 'rmem_label_components_workspace_bytes', 'rmem_label_components', 'rmem_label_component_stats',
       'rmem_label_clean')


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


def test_tile_and_workspace_queries(lib):
    from rmem_ocu_amd import components
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.rmem_label_components_tile(ctypes.byref(th), ctypes.byref(tw)) == 0 and th.value > 0 and tw.value > 0
    assert components.tile() == (th.value, tw.value)
    assert lib.rmem_label_components_tile(None, ctypes.byref(tw)) != 0 and b'null' in lib.rmem_last_error_string()
    one, two = lib.rmem_label_components_workspace_bytes(1, 480, 854), lib.rmem_label_components_workspace_bytes(2, 480, 854)
    assert one >= 480 * 854 * 20 + 256 * 3 * 4 and two == 2 * one
    assert lib.rmem_label_components_workspace_bytes(65535, 8192, 8192) == 65535 * lib.rmem_label_components_workspace_bytes(1, 8192, 8192)
    for n, H, W in ((1, 8193, 8192), (1, 1, (1 << 26) + 1), (0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.rmem_label_components_workspace_bytes(n, H, W) == 0, (n, H, W)


def test_entry_points_refuse_on_the_host(lib):
    """non-zero, a message that names the entry point, nothing launched (there is no GPU in this tier)"""
    fake = 4096                                                     # a non-null address that is never dereferenced on the host
    geometry = (((0, 4, 4), b'1..65535'), ((65536, 4, 4), b'1..65535'), ((1, 0, 4), b'positive'), ((1, 4, -1), b'positive'),
                ((1, 8193, 8193), b'2^26'))
    cases = []
    for k in (0, 5, 6):                                             # labels, roots, status
        args = [fake, 1, 4, 4, 8, fake, fake, None]
        args[k] = None
        cases.append(('rmem_label_components', args, b'null'))
    for (n, H, W), word in geometry:
        cases.append(('rmem_label_components', [fake, n, H, W, 8, fake, fake, None], word))
    for conn in (0, 6, -4, 9):
        cases.append(('rmem_label_components', [fake, 1, 4, 4, conn, fake, fake, None], b'connectivity'))
    for k in (0, 1, 6, 7):                                          # labels, roots, stats, table
        args = [fake, fake, 1, 4, 4, 8, fake, fake, None]
        args[k] = None
        cases.append(('rmem_label_component_stats', args, b'null'))
    for (n, H, W), word in geometry:
        cases.append(('rmem_label_component_stats', [fake, fake, n, H, W, 4, fake, fake, None], word))
    for conn in (0, 6, -4, 9):
        cases.append(('rmem_label_component_stats', [fake, fake, 1, 4, 4, conn, fake, fake, None], b'connectivity'))
    for k in range(5):                                              # src, dst, roots, stats, table
        args = [fake, fake, fake, fake, fake, 1, 4, 4, 0, 0, 0, None]
        args[k] = None
        cases.append(('rmem_label_clean', args, b'null'))
    for (n, H, W), word in geometry:
        cases.append(('rmem_label_clean', [fake, fake, fake, fake, fake, n, H, W, 0, 0, 0, None], word))
    cases.append(('rmem_label_clean', [fake, fake, fake, fake, fake, 1, 4, 4, -1, 0, 0, None], b'negative'))
    cases.append(('rmem_label_clean', [fake, fake, fake, fake, fake, 1, 4, 4, 0, -1, 1, None], b'negative'))
    for name, args, word in cases:
        rc = getattr(lib, name)(*args)
        msg = lib.rmem_last_error_string()
        assert rc != 0 and name.encode() + b':' in msg and word in msg, (name, args, msg)


def test_python_refusals():
    import torch
    from rmem_ocu_amd import components
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import clean_masks, object_fragments
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for call in (lambda: components.label_components(x), lambda: components.component_stats(x, x.int()), lambda: components.clean_labels(x),
                 lambda: components.object_fragments(x, 3), lambda: clean_masks(x), lambda: object_fragments(x, 3)):
        with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):      # a host tensor
            call()
    for call in (lambda: components.label_components(x.int()), lambda: components.clean_labels(x.float()), lambda: clean_masks(x.long())):
        with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):      # the wrong dtype
            call()
    for bad in (6, 0, 4.0, None, True):
        for call in (lambda: components.label_components(x, bad), lambda: components.component_stats(x, x.int(), bad),
                     lambda: components.clean_labels(x, connectivity=bad), lambda: components.object_fragments(x, 3, bad),
                     lambda: clean_masks(x, connectivity=bad)):
            with pytest.raises(RmemError, match='connectivity must be 4 or 8'):
                call()
    for bad in (-1, 2.5, None):
        with pytest.raises(RmemError, match='max_hole_area must be a non-negative integer'):
            components.clean_labels(x, max_hole_area=bad)
        with pytest.raises(RmemError, match='max_sprinkle_area must be a non-negative integer'):
            components.clean_labels(x, max_sprinkle_area=bad)
        with pytest.raises(RmemError, match='max_hole_area'):
            clean_masks(x, fill_holes=bad)
        with pytest.raises(RmemError, match='max_sprinkle_area'):
            clean_masks(x, remove_specks=bad)
    for out in (x[:1], x[0], torch.zeros(2, 4, 5, dtype=torch.uint8), np.zeros((2, 4, 4), dtype=np.uint8)):
        with pytest.raises(RmemError, match='out must be a tensor of the labels\' shape'):
            components.clean_labels(x, out=out)
    for bad in (0, 256, None, 2.5):
        with pytest.raises(RmemError, match=r'num_objs must be an integer in 1\.\.255'):
            components.object_fragments(x, bad)


def test_package_does_not_import_scipy_or_the_oracle():
    src = open(os.path.join(ROOT, 'rmem_ocu_amd', 'components.py')).read()
    assert 'scipy' not in src and 'oracle' not in src and 'ref_cpu' not in src
