"""The ring simplifier without a GPU: the sequential restatement (polysimplify_ref) on rings whose kept vertices are worked out
by hand, the contract's properties on seeded traced maps (subsequence, anchors, every dropped vertex within the tolerance in exact
rationals, T = 0, T = 1024), the far-pixel property through the fill restatement, the new symbols and host queries, every refusal
of the entry point and of the Python functions, and the degenerate filter and the 'area' rule driven from reference rings."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import components_ref
import polyfill_ref
import polygons_ref as P
import polysimplify_ref as S
from conftest import ROOT


def _kept(ring, T):
    return S.simplify_ring(ring, T)


# ---------------------------------------------------------------------------------------------------------- hand-checked rings
SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]
BUMP = [(0, 0), (5, 1), (10, 0), (10, 10), (0, 10)]                  # the bump is 1 pixel from the segment (0, 0) - (10, 0)
SADDLE = [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]


def test_pixel_square():
    """the corners 1 and 3 are 0.707 pixels from the diagonal of the anchors 0 and 2"""
    assert _kept(SQUARE, 8) == [0, 1, 2, 3]
    assert _kept(SQUARE, 11) == [0, 1, 2, 3]                        # 0.6875 < 0.7071
    assert _kept(SQUARE, 12) == [0, 2]                              # 0.75
    assert _kept(SQUARE, 16) == [0, 2]


def test_bump_below_at_and_above_the_threshold():
    """key = 100 against floor(100 T^2 / 256): the comparison is strict, a vertex AT the tolerance is dropped"""
    assert _kept(BUMP, 15) == [0, 1, 2, 3, 4]
    assert _kept(BUMP, 16) == [0, 2, 3, 4]
    assert _kept(BUMP, 17) == [0, 2, 3, 4]


def test_one_two_and_three_vertices():
    assert _kept([(7, 9)], 0) == [0] and _kept([(7, 9)], 1024) == [0]
    assert _kept([(7, 9), (7, 9)], 5) == [0, 1] and _kept([(0, 0), (3, 0)], 1024) == [0, 1]
    tri = [(0, 0), (4, 0), (4, 3)]                                  # vertex 1 is 12 / 5 = 2.4 pixels from the segment 0 - 2
    assert _kept(tri, 38) == [0, 1, 2] and _kept(tri, 39) == [0, 2]


def test_equal_vertices_and_the_point_segment():
    """all equal: every distance to p_0 is 0, so B = 1, and DP(1, k) measures against a segment of length 0"""
    assert _kept([(3, 3)] * 5, 0) == [0, 1] and _kept([(3, 3)] * 5, 1024) == [0, 1]
    assert S.key_thr((1, 1), (1, 1), (2, 3), 16) == (5, 1) and S.key_thr((1, 1), (1, 1), (2, 3), 40) == (5, 6)
    # beyond either end the distance is to the end point, times L
    assert S.key_thr((0, 0), (4, 0), (-3, 4), 0) == (25 * 16, 0) and S.key_thr((0, 0), (4, 0), (7, 4), 0) == (25 * 16, 0)
    assert S.key_thr((0, 0), (4, 0), (2, 3), 16) == (144, 16)


def test_saddle_ring_with_a_repeated_vertex():
    assert _kept(SADDLE, 0) == list(range(8))
    assert _kept(SADDLE, 7) == list(range(8))                       # (1, 1) is 0.447 pixels from the segment (1, 0) - (2, 2)
    assert _kept(SADDLE, 11) == [0, 1, 4, 5]                        # ... and (1, 0) 0.707 from the diagonal of the anchors
    assert _kept(SADDLE, 16) == [0, 4]


def test_both_tie_rules():
    assert _kept([(1, 1), (4, 1), (1, 4)], 1024) == [0, 1]           # two farthest vertices: the first is the anchor
    # vertices 2 and 3 are both 2 pixels from the segment 1 - 0: 2 wins, and 3 is then 1.099 pixels from the segment 2 - 0
    assert _kept([(0, 0), (10, 0), (7, 2), (3, 2)], 24) == [0, 1, 2]


def test_teeth_recursion_is_as_deep_as_the_ring_is_long():
    for k in (30, 100):
        ring = S.teeth(k)
        kept, depth = S.simplify_ring(ring.tolist(), 8, with_depth=True)
        assert len(ring) == 2 * k + 3 and depth >= 2 * k - 2 and len(kept) >= 2 * k
    assert len(S.teeth(30, pad=1)) == 64 and len(S.teeth(31)) == 65


# ------------------------------------------------------------------------------------------------- properties on traced maps
def _neighbours(kept, k):
    """for every dropped index its kept neighbours (i, j), j = k meaning vertex 0 again"""
    out = {}
    for i, j in zip(kept, kept[1:] + [k]):
        for m in range(i + 1, j):
            out[m] = (i, j)
    return out


def test_contract_properties_on_random_maps():
    rng = np.random.default_rng(31)
    for _ in range(300):
        K, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 12)), int(rng.integers(1, 12))
        frame = rng.integers(0, K + 2, size=(H, W), dtype=np.uint8)
        for conn in (4, 8):
            for r in P.trace(frame, K, conn):
                p = [tuple(v) for v in r['verts'].tolist()]
                k = len(p)
                d2 = [(x - p[0][0]) ** 2 + (y - p[0][1]) ** 2 for x, y in p]
                B = d2.index(max(d2[1:]), 1)
                for T in (0, 4, 8, 16, 23, 40, 1024):
                    kept = _kept(p, T)
                    assert kept == sorted(set(kept)) and kept[0] == 0 and B in kept and kept[-1] < k
                    for m, (i, j) in _neighbours(kept, k).items():
                        assert S.within(p[i], p[j % k], p[m], Fraction(T, 16)), (p, T, m)
                    if T == 1024:
                        assert kept == [0, B]                       # nothing in an 11 x 11 frame is 64 pixels from anything
                    if T == 0:                                      # exactly the vertices on their neighbours' segment leave
                        assert all(S.within(p[i], p[j % k], p[m], Fraction(0)) for m, (i, j) in _neighbours(kept, k).items())


def test_arrays_and_status():
    stack = P.noise(5, 2, 9, 11, 3)
    rings, verts, counts = P.arrays(stack, 2, 8)
    rs, vs, cs = S.simplify_arrays(rings, verts, counts, 16)
    R, V = int(counts[1]), int(counts[2])
    assert cs.tolist() == [V, R, len(vs), 0] and rs.shape == (R, 8) and rs.dtype == vs.dtype == np.int32
    assert np.array_equal(rs[:, [0, 1, 4, 5, 6]], rings[:, [0, 1, 4, 5, 6]]) and np.array_equal(rs[:, 7], rings[:, 3])
    assert np.array_equal(rs[:, 2], np.cumsum(rs[:, 3]) - rs[:, 3]) and rs[:, 3].sum() == len(vs) < V
    assert S.simplify_arrays(rings, verts, [77, 0, 0, 1], 16)[2].tolist() == [0, 0, 0, 1]
    assert S.simplify_arrays(rings, verts, counts, 16, max_rings=R - 1)[2].tolist() == [V, 0, 0, S.ST_TABLE]
    assert S.simplify_arrays(rings, verts, counts, 16, max_verts=V - 1)[2].tolist() == [V, 0, 0, S.ST_TABLE]
    bad = rings.copy()
    bad[1, 3] = 0
    rb, vb, cb = S.simplify_arrays(bad, verts, counts, 16)
    assert cb[3] == S.ST_RING and rb[1, 3] == 0 and rb[1, 7] == 0 and np.array_equal(rb[2:, 3], rs[2:, 3])
    assert len(vb) == len(vs) - rs[1, 3]


# -------------------------------------------------------------------------------------------------------- the far-pixel property
@functools.lru_cache(maxsize=None)
def _traced(name, shape, K, conn):
    a = S.content(name, shape, K)
    return a, P.arrays(a, K, conn)


def _filled_back(name, shape, K, conn, tolerance):
    a, (rings, verts, counts) = _traced(name, shape, K, conn)
    rs, vs, cs = S.simplify_arrays(rings, verts, counts, S.steps(tolerance))
    assert cs[3] == 0
    n, H, W = shape
    return a, polyfill_ref.paint_stack(S.shapes(rs, vs, n, K), H, W)


@pytest.mark.parametrize('tolerance', [0.5, 1.0, 1.5, 2.5])
@pytest.mark.parametrize('conn', [4, 8])
def test_far_pixels_keep_their_value_blobs(conn, tolerance):
    """smooth 3-object blobs: at least a fifth of the pixels are far, and not one of them changes"""
    shape, K = (2, 67, 133), 3
    a, back = _filled_back('blobs', shape, K, conn, tolerance)
    far = S.far_pixels(a, K, tolerance)
    assert far.mean() >= 0.2, far.mean()
    assert np.array_equal(back[far], a[far])
    assert (back != a).any() or tolerance < 1                       # the simplification does move boundary pixels


@pytest.mark.parametrize('name', ['speckle', 'others', 'concentric', 'nest', 'noise'])
def test_far_pixels_keep_their_value_other_contents(name):
    shape, K = (2, 23, 37), 10
    for conn in (4, 8):
        for tolerance in (0.5, 1.0, 2.5):
            a, back = _filled_back(name, shape, K, conn, tolerance)
            far = S.far_pixels(a, K, tolerance)
            obj = np.where(a > K, 0, a)
            assert np.array_equal(back[far], obj[far]), (name, conn, tolerance)


def test_tolerance_zero_fills_back_exactly():
    for name in ('blobs', 'speckle', 'noise'):
        a, back = _filled_back(name, (2, 23, 37), 10, 8, 0)
        assert np.array_equal(back, np.where(a > 10, 0, a))


# ------------------------------------------------------------------------------------------------------------------ the library
NEW = ('rmem_polygon_simplify_short_max', 'rmem_polygon_simplify_workspace_bytes', 'rmem_polygon_simplify')


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
    for name, value in (('RMEM_SIMPLIFY_ST_TABLE', polygons.SIMPLIFY_ST_TABLE), ('RMEM_SIMPLIFY_ST_RING', polygons.SIMPLIFY_ST_RING)):
        assert re.search(r'#define %s %d\b' % (name, value), text), name
    assert (polygons.SIMPLIFY_ST_TABLE, polygons.SIMPLIFY_ST_RING) == (S.ST_TABLE, S.ST_RING)
    assert polygons.SIMPLIFY_ST_TABLE & 7 == 0 and polygons.SIMPLIFY_ST_RING & 7 == 0          # clear of the tracer's bits
    assert polygons.TOLERANCE_STEPS == 16 and polygons.MAX_TOLERANCE == 64
    assert lib.rmem_abi_version() == _lib.ABI_VERSION == 15


def test_host_queries(lib):
    from rmem_ocu_amd import polygons
    short = lib.rmem_polygon_simplify_short_max()
    assert short >= 4 and polygons.short_max() == short
    q = lib.rmem_polygon_simplify_workspace_bytes
    small, more_verts, more_rings = q(1000, 4000), q(1000, 104000), q(101000, 4000)
    assert small > 0 and small % 16 == 0
    assert 32 * 100000 <= more_verts - small <= 32 * 100000 + 256 and 24 * 100000 <= more_rings - small <= 24 * 100000 + 1024
    assert q(2 ** 31 - 1, 2 ** 31 - 1) > 56 * (2 ** 31 - 1)
    for MR, MV in ((0, 8), (8, 0), (-1, 8), (8, -5), (2 ** 31, 8), (8, 2 ** 31)):
        assert q(MR, MV) == 0, (MR, MV)


def test_entry_point_refuses_on_the_host(lib):
    """non-zero, a message that names the entry point, nothing launched (there is no GPU in this tier)"""
    fake = 4096
    need = lib.rmem_polygon_simplify_workspace_bytes(16, 64)

    def args(**kw):
        a = dict(rings=fake, verts=fake, counts=fake, max_rings=16, max_verts=64, T=16, workspace=fake, nbytes=need, rings_out=fake,
                 verts_out=fake, counts_out=fake, stream=None)
        a.update(kw)
        return list(a.values())

    cases = [(args(**{k: None}), b'null') for k in ('rings', 'verts', 'counts', 'workspace', 'rings_out', 'verts_out', 'counts_out')]
    cases += [(args(max_rings=v), b'1..2^31-1') for v in (0, -1, 2 ** 31)] + [(args(max_verts=v), b'1..2^31-1') for v in (0, -7, 2 ** 31)]
    cases += [(args(T=v), b'0..1024') for v in (-1, 1025, 2 ** 20)]
    cases += [(args(nbytes=need - 1), b'smaller'), (args(nbytes=0), b'smaller'), (args(workspace=fake + 8), b'aligned')]
    for a, word in cases:
        rc = lib.rmem_polygon_simplify(*a)
        msg = lib.rmem_last_error_string()
        assert rc != 0 and b'rmem_polygon_simplify:' in msg and word in msg, (a, msg)


def test_python_refusals():
    import torch
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import polygon_results
    rings, verts, counts = torch.zeros(4, 8, dtype=torch.int32), torch.zeros(16, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for bad in (-0.1, 64.5, float('nan'), float('inf'), None, '1', True):
        with pytest.raises(RmemError, match=r'tolerance must be a finite number in 0\.\.64'):
            polygons.simplify(rings, verts, counts, bad)
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for bad in (-1, 65, float('nan'), '2', True):
        for call in (lambda: polygons.trace_label_stack(x, 3, tolerance=bad), lambda: polygon_results(x, 3, tolerance=bad)):
            with pytest.raises(RmemError, match=r'tolerance must be a finite number in 0\.\.64'):
                call()
    for bad in ('remove', None, 0):
        with pytest.raises(RmemError, match='degenerate must be'):
            polygons.trace_label_stack(x, 3, degenerate=bad)
    for a in ((rings.long(), verts, counts), (rings, verts.float(), counts), (rings, verts, counts.short()), (rings.numpy(), verts, counts)):
        with pytest.raises(RmemError, match='must be an int32 tensor'):
            polygons.simplify(*a, 1.0)
    for a, name in (((rings[:, :7], verts, counts), 'rings'), ((rings.view(8, 4), verts, counts), 'rings'), ((rings[:0], verts, counts), 'rings'),
                    ((rings, verts.view(-1), counts), 'verts'), ((rings, verts.view(8, 4)[:, :2], counts), 'verts'),
                    ((rings, verts, counts[:3]), 'counts'), ((rings, verts, counts.view(2, 2)), 'counts'),
                    ((rings, verts, torch.zeros(8, dtype=torch.int32)[::2]), 'counts')):
        with pytest.raises(RmemError, match=f'{name} must be a contiguous'):
            polygons.simplify(*a, 1.0)
    with pytest.raises(RmemError, match='must be device tensors'):
        polygons.simplify(rings, verts, counts, 1.0)


# ----------------------------------------------------------------------------------- the degenerate filter and the area rule
FRAME = np.array([[1, 1, 1, 1, 1, 1, 0, 2, 0],
                  [1, 0, 0, 0, 0, 1, 0, 0, 0],
                  [1, 0, 0, 1, 0, 1, 0, 3, 3],
                  [1, 0, 0, 0, 0, 1, 0, 3, 3],
                  [1, 0, 0, 0, 0, 1, 0, 0, 0],
                  [1, 1, 1, 1, 1, 1, 0, 0, 0]], dtype=np.uint8)


def _grouped(stack, K, conn, T):
    from rmem_ocu_amd import polygons
    rings, verts, counts = P.arrays(stack, K, conn)
    rs, vs, _ = S.simplify_arrays(rings, verts, counts, T)
    roots = components_ref.roots(stack, conn)
    at = np.array([roots[r[0]].reshape(-1)[r[5] >> 2] for r in rs], dtype=np.int32)
    return polygons.group_rings(rs, vs, len(stack), K, roots_at_start=at)


def _area2(ring):
    ring = [tuple(int(c) for c in p) for p in ring]
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]))


def test_degenerate_filter_and_area_rule():
    from rmem_ocu_amd import polygons
    kept = _grouped(FRAME[None], 3, 8, 16)[0]
    # at one pixel every single-pixel square collapses to its diagonal; the 2 x 2 square and the big ring with its hole stay
    assert [len(p['exterior']) for p in kept[1]] == [4, 2] and [len(h) for h in kept[1][0]['holes']] == [4]
    assert [len(p['exterior']) for p in kept[2]] == [2] and [len(p['exterior']) for p in kept[3]] == [4]
    assert kept[1][0]['area2'] == 2 * (36 - 16) and kept[1][1]['area2'] == 2       # the traced pixel areas
    dropped = polygons.drop_degenerate(_grouped(FRAME[None], 3, 8, 16))[0]
    assert [len(p['exterior']) for p in dropped[1]] == [4] and dropped[2] == [] and len(dropped[3]) == 1
    assert [h.tolist() for h in dropped[1][0]['holes']] == [[[1, 1], [1, 5], [5, 5], [5, 1]]]
    # an exterior that goes takes its holes along; a degenerate hole goes alone
    frames = [{1: [{'exterior': np.array([[0, 0], [5, 5]]), 'area2': 9, 'holes': [np.array([[1, 1], [1, 3], [3, 3], [3, 1]])]},
                   {'exterior': np.array([[0, 0], [9, 0], [9, 9], [0, 9]]), 'area2': 9,
                    'holes': [np.array([[1, 1], [2, 2], [3, 3]]), np.array([[1, 1], [1, 3]]), np.array([[4, 4], [4, 6], [6, 6]])]}]}]
    out = polygons.drop_degenerate(frames)[0][1]
    assert len(out) == 1 and [h.tolist() for h in out[0]['holes']] == [[[4, 4], [4, 6], [6, 6]]]
    # 'area': the shoelace area of the listed rings, a float
    full = polygons.coco_polygons([dropped], (6, 9), 'rings', simplified=True)[0]
    drop = polygons.coco_polygons([dropped], (6, 9), 'drop', simplified=True)[0]
    assert full[1]['area'] == 36.0 - 16.0 and isinstance(full[1]['area'], float) and drop[1]['area'] == 36.0 and 'holes' not in drop[1]
    assert full[2] == {'size': [6, 9], 'segmentation': [], 'holes': [], 'area': 0.0} and full[3]['area'] == 4.0
    for name, shape in (('blobs', (1, 37, 61)), ('speckle', (1, 23, 37))):
        stack = S.content(name, shape, 5)
        frames = polygons.drop_degenerate(_grouped(stack, 5, 8, 24))
        for mode in ('rings', 'drop'):
            for k, e in polygons.coco_polygons(frames, shape[1:], mode, simplified=True)[0].items():
                rings = e['segmentation'] + (e['holes'] if mode == 'rings' else [])
                assert e['area'] == sum(_area2(np.array(r).reshape(-1, 2)) for r in rings) / 2.0
                assert all(len(r) >= 6 for r in rings)
    # without the flag nothing changes: the traced pixel count
    assert polygons.coco_polygons([_grouped(FRAME[None], 3, 8, 0)[0]], (6, 9), 'rings')[0][1]['area'] == 21


def test_package_does_not_import_the_restatement():
    for name in ('polygons.py', 'evaluator.py'):
        src = open(os.path.join(ROOT, 'rmem_ocu_amd', name)).read()
        assert 'polysimplify_ref' not in src and 'scipy' not in src
