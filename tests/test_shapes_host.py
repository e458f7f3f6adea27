"""The host side of the shape census without a GPU: the reference (tests/shapes_ref.py) against qhull, the device's hull method
(corner levels from row extents, as a serial chain and as the O(h^2) membership rule) against the reference's brute force,
shapes.props_from_tables against the reference on tables the reference built, the minimum-area rectangle's properties, and the
refusals that need no device."""
import functools
import math

import numpy as np
import pytest
import torch

import census_ref
import shapes_ref as R


@functools.lru_cache(maxsize=None)
def _masks():
    """small masks of every kind: noise at several densities, rectangles, discs, blobs, and the corner cases by hand"""
    rng = np.random.default_rng(20261020)
    out = []
    for k in range(60):
        H, W = int(rng.integers(1, 24)), int(rng.integers(1, 40))
        kind = k % 4
        if kind == 0:
            m = rng.random((H, W)) < (0.05, 0.3, 0.7)[k // 4 % 3]
        elif kind == 1:
            m = np.zeros((H, W), dtype=bool)
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            m[y:y + int(rng.integers(1, H + 1)), x:x + int(rng.integers(1, W + 1))] = True
        elif kind == 2:
            m = R.disc(H, W, rng.integers(0, H), rng.integers(0, W), float(rng.integers(1, 12)) + 0.5 * (k % 3))
        else:
            m = census_ref.blobs(k, 1, H, W, ids=(1, 2, 3))[0] == 1 + k % 3
        out.append(m)
    c = np.zeros((9, 11), dtype=bool)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True                # four corner pixels: levels between without a candidate
    stair = np.eye(13, dtype=bool)
    cee = np.zeros((12, 10), dtype=bool)
    cee[1:11, 2:9] = True
    cee[4:8, 5:9] = False
    two = np.zeros((20, 30), dtype=bool)
    two[1:3, 2:5] = True
    two[15:19, 22:29] = True
    out += [c, stair, stair[:, ::-1], cee, two, np.ones((1, 1), dtype=bool), np.ones((1, 17), dtype=bool), np.ones((17, 1), dtype=bool),
            np.ones((5, 7), dtype=bool), R.disc(64, 64, 31.5, 31.5, 30.0)]
    return tuple(m for m in out if m.any())


def _ext_rows(m):
    return R.extents(m[None].astype(np.uint8), 1)[0, 0]


def test_reference_hull_is_canonical_and_convex():
    for m in _masks():
        ring = R.hull(m)
        p = [tuple(int(t) for t in q) for q in ring]
        assert len(p) >= 4 and len(set(p)) == len(p)
        assert p[0] == min(p, key=lambda q: (q[1], q[0])) and p[1][1] == p[0][1] and p[1][0] > p[0][0], 'east along the top edge first'
        assert all(R._cross(a, b, c) > 0 for a, b, c in zip(p, p[1:] + p[:1], p[2:] + p[:2])), 'strictly convex, positive shoelace'
        assert R.area2(ring) >= 2 * int(m.sum())
        assert len(p) <= 2 * (np.nonzero(m.any(axis=1))[0].size + 1)


def test_reference_hull_against_qhull():
    from scipy import spatial
    for m in _masks():
        ys, xs = np.nonzero(m)
        pts = np.array(sorted({(int(x) + dx, int(y) + dy) for x, y in zip(xs, ys) for dx in (0, 1) for dy in (0, 1)}))
        q = spatial.ConvexHull(pts)
        qv = {tuple(int(t) for t in pts[i]) for i in q.vertices}    # qhull may keep collinear points
        assert {tuple(int(t) for t in v) for v in R.hull(m)} <= qv
        assert math.isclose(q.volume, R.area2(R.hull(m)) / 2.0, rel_tol=1e-9)


def test_level_method_equals_brute_force():
    for m in _masks():
        want = R.hull(m)
        e = _ext_rows(m)
        assert np.array_equal(R.hull_by_level_chains(e, m.shape[1]), want)
        assert np.array_equal(R.hull_by_level_membership(e, m.shape[1]), want)


def test_level_method_full_size():
    m = R.disc(480, 854, 240, 400, 230)
    want = R.hull(m)
    assert len(want) >= 100
    assert np.array_equal(R.hull_by_level_chains(_ext_rows(m), 854), want)


def _tables(stack, num):
    verts, off = R.hulls(stack, num)
    return R.moments(stack), verts, off


def _assert_props_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in w:
            a, b = g[k], w[k]
            assert sorted(a) == sorted(b)
            for name in ('area', 'mu', 'hull_area2', 'feret2'):
                assert a[name] == b[name] and type(a[name]) is type(b[name]), (k, name, a[name], b[name])
            assert a['hull'].dtype == np.int32 and np.array_equal(a['hull'], b['hull'])
            for name in ('centroid', 'orientation', 'major_axis', 'minor_axis', 'eccentricity', 'solidity', 'extent', 'min_rect', 'min_rect_area'):
                assert np.allclose(np.asarray(a[name], dtype=np.float64), np.asarray(b[name], dtype=np.float64), rtol=1e-12, atol=0.0), (k, name, a[name], b[name])
            assert a['min_rect'].dtype == np.float64 and a['min_rect'].shape == (4, 2)


@functools.lru_cache(maxsize=None)
def _stack():
    a = census_ref.blobs(11, 3, 37, 131, ids=(1, 2, 3, 4, 6))
    a[1][R.disc(37, 131, 18, 90, 14)] = 5
    a[2, 3, 7] = 7                                                  # a single pixel
    a[0][a[0] == 2] = 0                                             # object 2 is absent from frame 0
    return a


def test_props_from_tables_equals_reference():
    from rmem_ocu_amd.shapes import props_from_tables
    a = _stack()
    n, H, W = a.shape
    got = props_from_tables(*_tables(a, 7), n, 7, H, W)
    _assert_props_equal(got, R.stack_props(a, 7))
    assert 2 not in got[0] and 7 in got[2] and 7 not in got[0]
    one = got[2][7]
    assert one['area'] == 1 and one['centroid'] == (7.0, 3.0) and one['mu'] == (0, 0, 0) and one['orientation'] == 0.0
    assert one['major_axis'] == 0.0 and one['eccentricity'] == 0.0 and one['hull_area2'] == 2 and one['solidity'] == 1.0
    assert one['feret2'] == 2 and one['min_rect_area'] == 1.0 and one['hull'].tolist() == [[7, 3], [8, 3], [8, 4], [7, 4]]
    sq = [0, 40, 41, 42, 43, 44]                                    # ids beyond squeeze_idx's length are left out
    _assert_props_equal(props_from_tables(*_tables(a, 7), n, 7, H, W, squeeze_idx=sq), R.stack_props(a, 7, sq))


def test_props_of_a_tilted_bar():
    """a one-pixel diagonal: orientation +45 degrees from +x towards +y, eccentricity 1, and a rotated box thinner than the upright one"""
    from rmem_ocu_amd.shapes import props_from_tables
    a = np.eye(13, dtype=np.uint8)[None]
    p = props_from_tables(*_tables(a, 1), 1, 1, 13, 13)[0][1]
    assert math.isclose(p['orientation'], math.pi / 4) and math.isclose(p['eccentricity'], 1.0) and p['minor_axis'] == 0.0
    assert p['centroid'] == (6.0, 6.0) and p['extent'] == 13 / 169 and p['feret2'] == 2 * 13 * 13
    assert p['min_rect_area'] < 0.25 * 169


def test_min_rect_properties():
    from rmem_ocu_amd.shapes import _min_rect
    for m in _masks():
        ring = R.hull(m)
        p = [tuple(int(t) for t in q) for q in ring]
        corners, area = _min_rect(ring)
        want_area, edge, want_corners = R.min_rect(ring)
        tol = 1e-9 * math.hypot(*m.shape)
        assert abs(area - float(want_area)) <= tol * math.hypot(*m.shape) and np.allclose(corners, want_corners, rtol=0, atol=tol)
        sides = np.roll(corners, -1, axis=0) - corners
        assert abs(abs(sides[0, 0] * sides[1, 1] - sides[0, 1] * sides[1, 0]) - area) <= tol * math.hypot(*m.shape)
        assert abs(sides[0] @ sides[1]) <= tol * math.hypot(*m.shape), 'a rectangle'
        for q in p:                                                 # every hull vertex inside: on the inner side of all four sides
            for c, s in zip(corners, sides):
                assert (s[0] * (q[1] - c[1]) - s[1] * (q[0] - c[0])) / max(np.hypot(*s), 1e-300) >= -tol
        e = np.array(p[(edge + 1) % len(p)], dtype=np.float64) - np.array(p[edge], dtype=np.float64)
        assert abs(e[0] * sides[0, 1] - e[1] * sides[0, 0]) / np.hypot(*e) <= tol * math.hypot(*m.shape), 'one side along a hull edge'
        d = np.array(p[edge], dtype=np.float64) - corners[0]
        assert abs(sides[0, 0] * d[1] - sides[0, 1] * d[0]) / np.hypot(*sides[0]) <= tol, 'and through it'


def test_refusals_without_a_device():
    from rmem_ocu_amd import shapes
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import object_centroids, object_shapes, rotated_boxes
    host = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for fn in (shapes.label_moments, lambda t: shapes.row_extents(t, 3), lambda t: shapes.convex_hulls(t, 3), lambda t: shapes.region_props(t, 3),
               lambda t: object_shapes(t, 3), lambda t: object_centroids(t, 3), lambda t: rotated_boxes(t, 3)):
        with pytest.raises(RmemError, match='uint8 device tensor'):
            fn(host)
    for num in (0, 256, -1, 2.0, True):
        for fn in (shapes.row_extents, shapes.convex_hulls, shapes.region_props, object_centroids, rotated_boxes):
            with pytest.raises(RmemError, match='num_objs'):
                fn(host, num)
    for ws in (0, -5, 1.5, '1'):
        with pytest.raises(RmemError, match='workspace_bytes'):
            shapes.convex_hulls(host, 3, workspace_bytes=ws)
    with pytest.raises(RmemError, match='moments'):
        shapes.props_from_tables(np.zeros((2, 256, 5), dtype=np.int64), np.zeros((0, 2), dtype=np.int32), np.zeros(7, dtype=np.int32), 2, 3, 8, 8)


def test_entry_points_refuse_on_the_host():
    """bad arguments never reach a launch: null pointers, n, sides above 16384, num outside 1..255"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    p = 4096                                                        # never dereferenced: every call below is refused first
    def refused(rc, text):
        assert rc != 0 and text in L.rmem_last_error_string(), L.rmem_last_error_string()
    refused(L.rmem_label_moments(None, 1, 8, 8, 1, p, p, None), b'null pointer')
    refused(L.rmem_label_moments(p, 1, 8, 8, 1, None, None, None), b'null pointer')
    refused(L.rmem_label_moments(p, 0, 8, 8, 1, p, p, None), b'1..65535')
    refused(L.rmem_label_moments(p, 65536, 8, 8, 1, p, p, None), b'1..65535')
    refused(L.rmem_label_moments(p, 1, 16385, 8, 1, p, p, None), b'16384')
    refused(L.rmem_label_moments(p, 1, 8, 16385, 1, p, p, None), b'16384')
    refused(L.rmem_label_moments(p, 1, 16384, 8192, 1, p, p, None), b'2^26')
    refused(L.rmem_label_moments(p, 1, 0, 8, 1, p, p, None), b'16384')
    refused(L.rmem_label_moments(p, 1, 8, 8, 0, None, p, None), b'1..255')
    refused(L.rmem_label_moments(p, 1, 8, 8, 256, p, p, None), b'1..255')
    refused(L.rmem_label_hull_count(None, 1, 8, 8, 1, p, p, None), b'null pointer')
    refused(L.rmem_label_hull_count(p, 1, 8, 8, 1, p, None, None), b'null pointer')
    refused(L.rmem_label_hull_count(p, 0, 8, 8, 1, p, p, None), b'1..65535')
    refused(L.rmem_label_hull_count(p, 1, 16385, 8, 1, p, p, None), b'16384')
    refused(L.rmem_label_hull_count(p, 1, 8, 8, 256, p, p, None), b'1..255')
    refused(L.rmem_label_hull_offsets(None, 4, None), b'null pointer')
    refused(L.rmem_label_hull_offsets(p, 0, None), b'objects')
    refused(L.rmem_label_hull_write(p, p, 1, 8, 8, 1, None, p, 8, None), b'null pointer')
    refused(L.rmem_label_hull_write(p, p, 1, 8, 16385, 1, p, p, 8, None), b'16384')
    refused(L.rmem_label_hull_write(p, p, 1, 8, 8, 0, p, p, 8, None), b'1..255')
    refused(L.rmem_label_hull_write(p, p, 1, 8, 8, 1, p, p, 0, None), b'capacity')
    refused(L.rmem_label_hull_write(p, p, 70000, 8, 8, 1, p, p, 8, None), b'1..65535')
