"""The polygon tracer without a GPU: the sequential restatement (polygons_ref) against maps whose rings, vertices and area2 are
written out by hand, the contract's properties on seeded random maps (round trip, piece and hole counts by scipy, area), the new
symbols, the workspace query, every refusal of the entry point and of the Python functions, and trace_label_stack's grouping and
parent assignment driven from reference rings."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import components_ref
import polygons_ref as R
from conftest import ROOT


def _rings(frame, num_objs, connectivity):
    return [(r['value'], r['start'], r['edges'], r['area2'], [tuple(v) for v in r['verts'].tolist()])
            for r in R.trace(np.array(frame, dtype=np.uint8), num_objs, connectivity)]


@pytest.mark.parametrize('connectivity', [4, 8])
def test_one_pixel(connectivity):
    assert _rings([[1]], 1, connectivity) == [(1, 0, 4, 2, [(0, 0), (1, 0), (1, 1), (0, 1)])]


def test_two_diagonal_pixels_are_one_ring_under_8():
    """the ring passes the saddle (1, 1) twice"""
    assert _rings([[1, 0], [0, 1]], 1, 8) == [(1, 0, 8, 4, [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)])]


def test_two_diagonal_pixels_are_two_rings_under_4():
    assert _rings([[1, 0], [0, 1]], 1, 4) == [(1, 0, 4, 2, [(0, 0), (1, 0), (1, 1), (0, 1)]),
                                             (1, 12, 4, 2, [(1, 1), (2, 1), (2, 2), (1, 2)])]


@pytest.mark.parametrize('connectivity', [4, 8])
def test_frame_with_a_hole(connectivity):
    """3 x 4 with a 1 x 2 hole: the hole's start edge 6 (the bottom of pixel (0, 1), heading west) is no corner"""
    frame = [[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 1]]
    assert _rings(frame, 1, connectivity) == [(1, 0, 14, 24, [(0, 0), (4, 0), (4, 3), (0, 3)]),
                                              (1, 6, 6, -4, [(1, 1), (1, 2), (3, 2), (3, 1)])]


@pytest.mark.parametrize('connectivity', [4, 8])
def test_hole_between_two_objects_is_no_ring(connectivity):
    frame = [[1, 1, 2, 2], [1, 0, 0, 2], [1, 1, 2, 2]]
    assert _rings(frame, 2, connectivity) == [
        (1, 0, 12, 10, [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (2, 2), (2, 3), (0, 3)]),
        (2, 8, 12, 10, [(2, 0), (4, 0), (4, 3), (2, 3), (2, 2), (3, 2), (3, 1), (2, 1)])]


def test_object_on_the_frames_edge_side_by_side_and_other_values():
    assert _rings([[0, 0, 0], [0, 0, 3]], 3, 8) == [(3, 20, 4, 2, [(2, 1), (3, 1), (3, 2), (2, 2)])]
    assert _rings([[1, 2]], 2, 4) == [(1, 0, 4, 2, [(0, 0), (1, 0), (1, 1), (0, 1)]), (2, 4, 4, 2, [(1, 0), (2, 0), (2, 1), (1, 1)])]
    assert _rings([[1, 7]], 2, 8) == [(1, 0, 4, 2, [(0, 0), (1, 0), (1, 1), (0, 1)])]         # 7 is above num_objs: not an object
    assert _rings([[7, 7], [7, 255]], 6, 8) == []
    # a value above num_objs inside an object is a hole like the background; the start edge of a one-pixel hole is a corner
    assert _rings([[1, 1, 1], [1, 9, 1], [1, 1, 1]], 1, 8) == [(1, 0, 12, 18, [(0, 0), (3, 0), (3, 3), (0, 3)]),
                                                              (1, 6, 4, -2, [(2, 1), (1, 1), (1, 2), (2, 2)])]


def test_arrays_layout():
    stack = np.array([[[1, 0], [0, 1]], [[0, 0], [0, 0]], [[2, 2], [2, 2]]], dtype=np.uint8)
    rings, verts, counts = R.arrays(stack, 2, 4)
    assert rings.dtype == np.int32 and verts.dtype == np.int32 and counts.tolist() == [16, 3, 12, 0]
    assert rings.tolist() == [[0, 1, 0, 4, 2, 0, 4, 0], [0, 1, 4, 4, 2, 12, 4, 0], [2, 2, 8, 4, 8, 0, 8, 0]]
    assert verts[8:].tolist() == [[0, 0], [2, 0], [2, 2], [0, 2]]
    rings, verts, counts = R.arrays(stack[1:2], 2, 8)
    assert rings.shape == (0, 8) and verts.shape == (0, 2) and counts.tolist() == [0, 0, 0, 0]


FOUR = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
EIGHT = [[1, 1, 1], [1, 1, 1], [1, 1, 1]]


def test_contract_properties_on_random_maps():
    """300 seeded maps, 1..3 objects, H and W in 1..11, both connectivities: rasterising the rings reproduces every mask, the
    outer rings are the pieces, the holes the enclosed pieces of the rest under the dual connectivity, area2 sums to 2 x area"""
    rng = np.random.default_rng(20)
    for _ in range(300):
        K, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 12)), int(rng.integers(1, 12))
        frame = rng.integers(0, K + 2, size=(H, W), dtype=np.uint8)                     # K + 1 is a value above num_objs
        for conn in (4, 8):
            rings = R.trace(frame, K, conn)
            assert [r['start'] for r in rings] == sorted(r['start'] for r in rings)
            assert sum(r['edges'] for r in rings) == len(R.edges(frame, K))
            for v in range(1, K + 1):
                mask = frame == v
                mine = [r for r in rings if r['value'] == v]
                assert np.array_equal(R.rasterise(rings, v, H, W), mask), (frame, conn, v)
                assert sum(r['area2'] for r in mine) == 2 * int(mask.sum())
                assert sum(r['area2'] > 0 for r in mine) == ndimage.label(mask, structure=EIGHT if conn == 8 else FOUR)[1]
                rest, pieces = ndimage.label(~np.pad(mask, 1), structure=FOUR if conn == 8 else EIGHT)
                assert sum(r['area2'] < 0 for r in mine) == pieces - 1                  # all but the piece that holds the padding
            for r in rings:
                v = r['verts']
                d = np.roll(v, -1, axis=0) - v
                assert len(v) >= 4 and (np.count_nonzero(d, axis=1) == 1).all()         # axis-parallel steps
                assert (np.abs(np.sign(d) - np.sign(np.roll(d, -1, axis=0))).sum(axis=1) > 0).all()      # no collinear vertex


def test_contents_are_what_they_claim():
    s = R.serpentine(1, 9, 12)[0]
    rings = R.trace(s, 1, 4)
    assert len(rings) == 1 and rings[0]['edges'] == len(R.edges(s, 1)) and rings[0]['area2'] == 2 * int(s.sum())
    c = R.checkerboard(1, 6, 7)[0]
    for v in (1, 2):
        mine = [r for r in R.trace(c, 2, 8) if r['value'] == v]
        assert sum(r['area2'] > 0 for r in mine) == 1 and sum(r['edges'] for r in mine) == 4 * int((c == v).sum())
        assert all(r['area2'] == 2 for r in R.trace(c, 2, 4))
    rings = R.trace(R.concentric(1, 13, 15)[0], 2, 8)
    assert sum(r['area2'] > 0 for r in rings) == 4 and sum(r['area2'] < 0 for r in rings) == 3
    rings = R.trace(R.nest(1, 14, 16)[0], 3, 8)
    assert [(r['value'], r['area2'] > 0) for r in rings] == [(1, True), (1, False), (2, True), (2, False), (3, True)]


# ------------------------------------------------------------------------------------------------------------------ the library
NEW = ('rmem_label_polygons_unit', 'rmem_label_polygons_workspace_bytes', 'rmem_label_polygons')


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from rmem_ocu_amd import _lib, polygons
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rmem.h')).read(), flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/rmem.h'
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name, value in (('RMEM_POLY_ST_CAPACITY', polygons.ST_CAPACITY), ('RMEM_POLY_ST_LINK', polygons.ST_LINK),
                        ('RMEM_POLY_ST_ORDER', polygons.ST_ORDER)):
        assert re.search(r'#define %s %d\b' % (name, value), text), name
    assert polygons.ST_CAPACITY == R.ST_CAPACITY
    assert lib.rmem_abi_version() == _lib.ABI_VERSION


def test_unit_and_workspace_query(lib):
    from rmem_ocu_amd import polygons
    unit = lib.rmem_label_polygons_unit()
    assert unit >= 1 and polygons.unit() == unit
    q = lib.rmem_label_polygons_workspace_bytes
    small, large = q(1, 480, 854, 1000), q(1, 480, 854, 101000)
    assert small > 0 and small % 16 == 0 and 40 * 100000 <= large - small <= 40 * 100000 + 1024      # 40 bytes per edge of capacity
    assert q(2, 480, 854, 1000) - small >= 4 * 480 * ((854 + unit - 1) // unit)                      # 4 per walk unit
    assert q(65535, 8192, 8192, 2 ** 31 - 1) > 40 * (2 ** 31 - 1)
    for n, H, W, M in ((1, 8193, 8192, 64), (1, 1, (1 << 26) + 1, 64), (0, 4, 4, 64), (65536, 4, 4, 64), (1, 0, 4, 64), (1, 4, -1, 64),
                       (1, 4, 4, 3), (1, 4, 4, 0), (1, 4, 4, -8)):
        assert q(n, H, W, M) == 0, (n, H, W, M)


def test_entry_point_refuses_on_the_host(lib):
    """non-zero, a message that names the entry point, nothing launched (there is no GPU in this tier)"""
    fake = 4096                                                     # a non-null address that is never dereferenced on the host
    need = lib.rmem_label_polygons_workspace_bytes(1, 4, 4, 64)

    def args(**kw):
        a = dict(labels=fake, n=1, H=4, W=4, num_objs=3, connectivity=8, max_edges=64, workspace=fake, nbytes=need, rings=fake,
                 verts=fake, counts=fake, stream=None)
        a.update(kw)
        return list(a.values())

    cases = [(args(**{k: None}), b'null') for k in ('labels', 'workspace', 'rings', 'verts', 'counts')]
    cases += [(args(n=0), b'1..65535'), (args(n=65536), b'1..65535'), (args(H=0), b'positive'), (args(W=-1), b'positive'),
              (args(H=8193, W=8193, nbytes=1 << 40), b'2^26')]
    cases += [(args(num_objs=k), b'num_objs') for k in (0, 256, -1)]
    cases += [(args(connectivity=c), b'connectivity') for c in (0, 6, -4, 9)]
    cases += [(args(max_edges=m), b'max_edges') for m in (3, 0, -1)]
    cases += [(args(nbytes=need - 1), b'smaller'), (args(nbytes=0), b'smaller'), (args(workspace=fake + 4), b'aligned')]
    for a, word in cases:
        rc = lib.rmem_label_polygons(*a)
        msg = lib.rmem_last_error_string()
        assert rc != 0 and b'rmem_label_polygons:' in msg and word in msg, (a, msg)


def test_python_refusals():
    import torch
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import polygon_results
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for call in (lambda: polygons.trace(x, 3), lambda: polygons.trace_label_stack(x, 3), lambda: polygon_results(x, 3),
                 lambda: polygons.trace(x.int(), 3), lambda: polygons.trace_label_stack(np.zeros((2, 4, 4), dtype=np.uint8), 3)):
        with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
            call()
    for bad in (0, 256, None, 2.5, True):
        for call in (lambda: polygons.trace(x, bad), lambda: polygons.trace_label_stack(x, bad), lambda: polygon_results(x, bad)):
            with pytest.raises(RmemError, match=r'num_objs must be an integer in 1\.\.255'):
                call()
    for bad in (6, 0, 4.0, None, True):
        for call in (lambda: polygons.trace(x, 3, bad), lambda: polygons.trace_label_stack(x, 3, bad),
                     lambda: polygon_results(x, 3, connectivity=bad)):
            with pytest.raises(RmemError, match='connectivity must be 4 or 8'):
                call()
    with pytest.raises(RmemError, match='holes must be'):
        polygon_results(x, 3, holes='fill')


def test_default_max_edges_is_an_estimate_far_below_the_bound():
    from rmem_ocu_amd import polygons
    assert polygons.default_max_edges(1, 1, 1) == 4 and polygons.default_max_edges(3, 1, 1) == 12
    for n, H, W in ((1, 480, 854), (64, 480, 854), (2, 37, 131)):
        m = polygons.default_max_edges(n, H, W)
        assert n * (H * W // 4) <= m <= n * H * W
    a = np.zeros((480, 854), dtype=np.uint8)
    a[100:300, 200:600] = 1                                         # a blob's outline is a small part of it
    assert 10 * len(R.edges(a, 1)) < polygons.default_max_edges(1, 480, 854)
    assert polygons.default_max_edges(65535, 8192, 8192) == 2 ** 31 - 1


# -------------------------------------------------------------------------------------------------- grouping, on the host alone
NESTED = np.array([[1, 1, 1, 1, 1, 0, 2],
                   [1, 0, 0, 0, 1, 0, 0],
                   [1, 0, 1, 0, 1, 0, 2],
                   [1, 0, 0, 0, 1, 0, 2],
                   [1, 1, 1, 1, 1, 0, 0]], dtype=np.uint8)


def _grouped(stack, K, conn, **kw):
    from rmem_ocu_amd import polygons
    rings, verts, _ = R.arrays(stack, K, conn)
    roots = components_ref.roots(stack, conn)
    at = np.array([roots[r[0]].reshape(-1)[r[5] >> 2] for r in rings], dtype=np.int32)
    return polygons.group_rings(rings, verts, len(stack), K, roots_at_start=at, **kw)


def test_grouping_and_parents():
    from rmem_ocu_amd import polygons
    stack = np.stack([NESTED, np.zeros_like(NESTED)])
    frames = _grouped(stack, 3, 8)
    assert len(frames) == 2 and list(frames[0]) == [1, 2, 3] and frames[1] == {1: [], 2: [], 3: []}
    ring, island = frames[0][1]                                     # the pieces in the order of their first pixels
    assert ring['exterior'].tolist() == [[0, 0], [5, 0], [5, 5], [0, 5]] and ring['exterior'].dtype == np.int32
    assert [h.tolist() for h in ring['holes']] == [[[1, 1], [1, 4], [4, 4], [4, 1]]] and ring['area2'] == 2 * 16
    assert island == {'exterior': island['exterior'], 'area2': 2, 'holes': []} and island['exterior'].tolist() == [[2, 2], [3, 2], [3, 3], [2, 3]]
    assert [p['area2'] for p in frames[0][2]] == [2, 4] and frames[0][3] == []
    # un-squeezed keys; ids beyond squeeze_idx are left out
    assert list(_grouped(stack, 3, 8, squeeze_idx=[0, 7, 9])[0]) == [7, 9]
    # without parents: holes per object under the None key
    rings, verts, _ = R.arrays(stack, 3, 8)
    loose = polygons.group_rings(rings, verts, 2, 3)
    assert [p['area2'] for p in loose[0][1]] == [50, 2] and all(p['holes'] == [] for p in loose[0][1])
    assert [h.tolist() for h in loose[0][None]['holes'][1]] == [[[1, 1], [1, 4], [4, 4], [4, 1]]] and loose[0][None]['holes'][2] == []
    # a hole whose root is no outer ring's start is a bug that is named
    from rmem_ocu_amd._lib import RmemError
    with pytest.raises(RmemError, match='no outer ring'):
        polygons.group_rings(rings, verts, 2, 3, roots_at_start=np.full(len(rings), 33, dtype=np.int32))


@pytest.mark.parametrize('connectivity', [4, 8])
def test_grouping_on_random_maps(connectivity):
    """every hole lands in the piece that surrounds it: each polygon alone rasterises to one piece of its object"""
    rng = np.random.default_rng(7)
    structure = EIGHT if connectivity == 8 else FOUR
    for _ in range(40):
        H, W = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        stack = rng.integers(0, 3, size=(2, H, W), dtype=np.uint8)
        for f, fr in enumerate(_grouped(stack, 2, connectivity)):
            for v in (1, 2):
                pieces, count = ndimage.label(stack[f] == v, structure=structure)
                assert len(fr[v]) == count
                for k, p in enumerate(fr[v]):
                    own = [{'value': v, 'verts': p['exterior']}] + [{'value': v, 'verts': h} for h in p['holes']]
                    got = R.rasterise(own, v, H, W)
                    assert p['area2'] == 2 * int(got.sum()) and len(np.unique(pieces[got])) == 1 and (pieces == pieces[got][0]).sum() == got.sum()


def test_coco_shaping():
    from rmem_ocu_amd import polygons
    frames = _grouped(NESTED[None], 3, 8)
    full = polygons.coco_polygons(frames, (5, 7), 'rings')[0]
    assert full[1] == {'size': [5, 7], 'segmentation': [[0, 0, 5, 0, 5, 5, 0, 5], [2, 2, 3, 2, 3, 3, 2, 3]],
                       'holes': [[1, 1, 1, 4, 4, 4, 4, 1]], 'area': 17}
    assert full[3] == {'size': [5, 7], 'segmentation': [], 'holes': [], 'area': 0}
    drop = polygons.coco_polygons(frames, (5, 7), 'drop')[0]
    assert drop[1] == {'size': [5, 7], 'segmentation': [[0, 0, 5, 0, 5, 5, 0, 5], [2, 2, 3, 2, 3, 3, 2, 3]], 'area': 26}
    assert drop[2]['area'] == 3 and 'holes' not in drop[2]


def test_package_does_not_import_the_restatement():
    for name in ('polygons.py', 'evaluator.py'):
        src = open(os.path.join(ROOT, 'rmem_ocu_amd', name)).read()
        assert 'polygons_ref' not in src and 'scipy' not in src
