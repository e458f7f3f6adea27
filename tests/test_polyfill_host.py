"""The polygon fill, the part that needs no GPU: the restatement (tests/polyfill_ref.py) on hand cases and on the three seeded
properties it rests on (the round trip against the tracer's restatement, the partition by a triangle fan, the agreement with a
float crossing-number test), the layout of PackedPolygons against direct counts, every refusal of the Python layer and of the two
C entry points by message, the workspace query, and labels_from_polygons' listing with the fill stubbed by the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import polyfill_ref as P
import polygons_ref as R
from conftest import ROOT


def _set(mask):
    return sorted((int(y), int(x)) for y, x in np.argwhere(mask))


# ---------------------------------------------------------------------------------------------------------------- hand cases
def test_unit_square_fills_one_pixel():
    got = P.fill_rings([[(2, 1), (3, 1), (3, 2), (2, 2)]], 4, 5)
    assert _set(got) == [(1, 2)]
    assert _set(P.fill_rings([[2, 1, 3, 1, 3, 2, 2, 2]], 4, 5)) == [(1, 2)]          # the flat form


def test_corners_at_pixel_centres_fill_the_top_left_inclusive_set():
    got = P.fill_rings([[(1.5, 1.5), (4.5, 1.5), (4.5, 4.5), (1.5, 4.5)]], 7, 7)
    assert _set(got) == [(y, x) for y in (1, 2, 3) for x in (1, 2, 3)]               # centres 1.5 .. 3.5: left / top in, right / bottom out


def test_exterior_with_a_hole_in_either_orientation():
    ext = [(0, 0), (7, 0), (7, 6), (0, 6)]
    hole = [(2, 2), (5, 2), (5, 4), (2, 4)]
    want = np.ones((6, 7), dtype=bool)
    want[2:4, 2:5] = False
    for e in (ext, ext[::-1]):
        for h in (hole, hole[::-1]):
            assert np.array_equal(P.fill_rings([e, h], 6, 7), want)
            assert np.array_equal(P.fill_rings([h, e], 6, 7), want)


def test_triangle_outside_the_frame_fills_nothing():
    for ring in ([(-9, -9), (-2, -9), (-2, -1)], [(20, 3), (30, 3), (25, 30)], [(1, 40), (5, 40), (3, 44)], [(-5, 1), (-1, 2), (-3, 5)]):
        assert not P.fill_rings([ring], 8, 9).any()


def test_shared_edges_neither_overlap_nor_leave_a_gap():
    a, b = [(0.3, 0.2), (6.1, 7.7), (0.3, 7.7)], [(0.3, 0.2), (6.1, 0.2), (6.1, 7.7)]
    fa, fb = P.fill_rings([a], 9, 8), P.fill_rings([b], 9, 8)
    assert not (fa & fb).any()
    assert np.array_equal(fa | fb, P.fill_rings([[(0.3, 0.2), (6.1, 0.2), (6.1, 7.7), (0.3, 7.7)]], 9, 8))


def test_tie_cases_agree_with_the_crossing_number():
    for name, rings in P.tie_cases():
        assert np.array_equal(P.fill_rings(rings, 7, 9), P.crossing_number(rings, 7, 9)), name
    by_name = dict(P.tie_cases())
    assert not P.fill_rings(by_name['zero area, collinear'], 7, 9).any()
    assert not P.fill_rings(by_name['zero area, out and back'], 7, 9).any()
    assert not P.fill_rings(by_name['a ring listed twice cancels'], 7, 9).any()
    assert np.array_equal(P.fill_rings(by_name['repeated vertices'], 7, 9), P.fill_rings(by_name['vertices on pixel centres'], 7, 9))


# ---------------------------------------------------------------------------------------------------------------- seeded properties
def test_round_trip_against_the_tracer_restatement():
    """200 seeded maps, H and W in 1..11, 1..3 objects, both connectivities: the fill of the rings of value v is a == v"""
    rng = np.random.default_rng(2024)
    for k in range(200):
        H, W, objs = int(rng.integers(1, 12)), int(rng.integers(1, 12)), int(rng.integers(1, 4))
        a = rng.integers(0, objs + 1, size=(H, W))
        for conn in (4, 8):
            rings = R.trace(a, objs, conn)
            for v in range(1, objs + 1):
                got = P.fill([256 * r['verts'].astype(np.int64) for r in rings if r['value'] == v], H, W)
                assert np.array_equal(got, a == v), (k, conn, v)


def test_triangle_fan_covers_every_pixel_exactly_once():
    """300 fans round a centre that is a pixel centre, a pixel corner or fractional; H and W in 1..19"""
    rng = np.random.default_rng(7)
    for k in range(300):
        H, W = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        outline, triangles = P.triangle_fan(rng, H, W, ('centre', 'corner', 'fraction')[k % 3])
        cover = sum(P.fill_rings([t], H, W).astype(np.int64) for t in triangles)
        assert np.array_equal(cover, P.fill_rings([outline], H, W).astype(np.int64)), k


def test_agreement_with_a_float_crossing_number_test():
    """100 random polygons, self-intersecting ones and stars among them, every pixel of their frames"""
    rng = np.random.default_rng(11)
    pixels = 0
    for k in range(100):
        H, W = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        ring = P.star(rng, H, W) if k % 4 == 3 else P.random_polygon(rng, H, W)
        assert np.array_equal(P.fill_rings([ring], H, W), P.crossing_number([ring], H, W)), k
        pixels += H * W
    assert pixels > 5000


# ---------------------------------------------------------------------------------------------------------------- packing
def _direct(frames, H, W):
    """the shape table, the kept edges and the crossing prefix of frames[f] = [(value, [ring, ...])], counted one by one"""
    table, edges, shape_of, counts, plane = [], [], [], [], 0
    for f, shapes in enumerate(frames):
        for value, rings in shapes:
            q = [P.quantise(r) for r in rings]
            box = [0, 0, 0, 0]
            if q:
                allv = np.concatenate(q)
                xs = [x for x in range(W) if allv[:, 0].min() <= 256 * x + 128 < allv[:, 0].max()]
                ys = [y for y in range(H) if allv[:, 1].min() <= 256 * y + 128 < allv[:, 1].max()]
                if xs and ys:
                    box = [xs[0], ys[0], xs[-1] + 1, ys[-1] + 1]
            assert not P.fill(q, H, W)[:, :box[0]].any() and not P.fill(q, H, W)[:, box[2]:].any()
            assert not P.fill(q, H, W)[:box[1]].any() and not P.fill(q, H, W)[box[3]:].any()
            words = (box[3] - box[1]) * ((box[2] - box[0] + 31) // 32)
            if words:
                for r in q:
                    v = [(int(a), int(b)) for a, b in r]
                    for (X0, Y0), (X1, Y1) in zip(v, v[1:] + v[:1]):
                        c = sum(1 for y in range(H) if min(Y0, Y1) <= 256 * y + 128 < max(Y0, Y1))
                        if c:
                            edges.append((X0, Y0, X1, Y1))
                            shape_of.append(len(table))
                            counts.append(c)
            table.append((f, value, *box, plane))
            plane += words
    return table, edges, shape_of, [0] + list(np.cumsum(counts)), plane


def _clip():
    """three frames of shapes as (value, [float ring, ...]): fractional, off-frame, empty, a hole, a frame without shapes"""
    rng = np.random.default_rng(5)
    H, W = 19, 45
    f0 = [(3, [P.random_polygon(rng, H, W, 5)]), (200, [[(2, 2), (40.5, 2), (40.5, 17.25), (2, 17.25)], [(10, 5), (30, 5), (30, 12), (10, 12)]]),
          (7, []), (9, [[(-9.5, -9), (-2, -9), (-2, -1)]])]
    f2 = [(1, [P.star(rng, H, W)]), (255, [P.random_polygon(rng, H, W, 7), P.random_polygon(rng, H, W, 3)]), (1, [[(33.2, 0.1), (44.9, 0.3), (40, 18.8)]])]
    return [f0, [], f2], H, W


def test_packed_layout_against_a_direct_count():
    from rmem_ocu_amd import _lib, polygons
    frames, H, W = _clip()
    p = polygons.PackedPolygons(frames, (H, W))
    table, edges, shape_of, first, plane_words = _direct(frames, H, W)
    assert len(p) == p.nshapes == len(table) == 7 and tuple(p.shape) == (3, H, W)
    assert [tuple(int(v) for v in row) for row in p.table] == table
    assert p.edge_xy.tolist() == [list(e) for e in edges] and p.edge_shape.tolist() == shape_of
    assert p.edge_first.tolist() == first and p.crossings == first[-1] and p.nedges == len(edges)
    assert p.frame_shape.tolist() == [0, 4, 4, 7] and p.plane_words == plane_words
    assert p.where == [(0, 3), (0, 200), (0, 7), (0, 9), (2, 1), (2, 255), (2, 1)]
    assert tuple(p.table[2])[2:6] == (0, 0, 0, 0) and tuple(p.table[3])[2:6] == (0, 0, 0, 0)      # empty ring list; off the frame
    blob = np.frombuffer(p.buf.numpy().tobytes(), dtype=np.int32)
    E = len(edges)
    assert p.offsets == (0, 16 * E, 20 * E, 24 * E + 4) and blob.size == 6 * E + 1 + 4
    assert blob[:4 * E].reshape(-1, 4).tolist() == [list(e) for e in edges] and blob[4 * E:5 * E].tolist() == shape_of
    assert blob[5 * E:6 * E + 1].tolist() == first and blob[6 * E + 1:].tolist() == [0, 4, 4, 7]
    assert ctypes.sizeof(_lib.PolyShape) == 32 == polygons.SHAPE_DTYPE.itemsize and p.desc_bytes.numel() == 7 * 32
    d = _lib.PolyShape.from_buffer_copy(p.desc_bytes.numpy().tobytes()[32:64])
    assert (d.frame, d.value, d.x0, d.y0, d.x1, d.y1, d.plane) == table[1]
    assert ctypes.sizeof(_lib.PolyPass) == 56
    assert p.NOUN and set(p.STATUS_NAMES) == {1, 2, 4}
    assert p.frame_words.tolist() == [table[4][6], 0, plane_words - table[4][6]]


def _forms(rings):
    """one geometry (an exterior and holes as float [k, 2] arrays) in every form PackedPolygons takes"""
    ext, holes = rings[0], rings[1:]
    flat = [r.reshape(-1).tolist() for r in rings]
    return {
        'list of arrays': list(rings),
        'list of lists of pairs': [[tuple(p) for p in r.tolist()] for r in rings],
        'list of flat rings': flat,
        'array of rings': np.stack(rings) if len({len(r) for r in rings}) == 1 else list(rings),
        'polygon dict': {'exterior': ext, 'holes': list(holes), 'area2': 5},
        'list of polygon dicts': [{'exterior': ext, 'holes': list(holes)}],
        'coco entry': {'size': [19, 45], 'segmentation': [flat[0]], 'holes': flat[1:], 'area': 3},
    }


def test_every_shape_form_packs_to_identical_bytes():
    from rmem_ocu_amd import polygons
    H, W = 19, 45
    rings = [np.array([(2, 2), (40.5, 2), (40.5, 17.25), (2, 17.25)]), np.array([(10, 5), (30, 5), (30, 12.5), (10, 12)]),
             np.array([(32, 3.5), (38, 3), (38, 9), (32, 9)])]
    packs = {name: polygons.PackedPolygons([{4: form}, [(9, form), (2, form)]], (H, W)) for name, form in _forms(rings).items()}
    first = packs['list of arrays']
    assert first.nedges == 3 * 6 and first.crossings > 0                         # two edges of every ring cross a sample row
    for name, p in packs.items():
        assert p.buf.numpy().tobytes() == first.buf.numpy().tobytes(), name
        assert p.desc_bytes.numpy().tobytes() == first.desc_bytes.numpy().tobytes(), name
    one = rings[0]
    singles = [one, one.tolist(), [tuple(v) for v in one.tolist()], one.reshape(-1).tolist(), one.reshape(-1), [one], {'exterior': one},
               {'segmentation': [one.reshape(-1).tolist()]}]
    ref = polygons.PackedPolygons([{1: one}], (H, W))
    for k, s in enumerate(singles):
        q = polygons.PackedPolygons([[(1, s)]], (H, W))
        assert q.buf.numpy().tobytes() == ref.buf.numpy().tobytes() and q.desc_bytes.numpy().tobytes() == ref.desc_bytes.numpy().tobytes(), k
    ints = polygons.PackedPolygons([{1: np.array([(2, 2), (40, 2), (40, 17), (2, 17)], dtype=np.int32)}], (H, W))
    assert ints.edge_xy.tolist() == [[10240, 512, 10240, 4352], [512, 4352, 512, 512]]              # integers are exact; horizontals are dropped


def test_packing_quantises_like_the_reference():
    from rmem_ocu_amd import polygons
    rng = np.random.default_rng(3)
    ring = np.concatenate([P.random_polygon(rng, 30, 30, 6), [(1 + 1 / 512, 2 + 3 / 512), (7 + 5 / 512, 29.998046875)]])
    p = polygons.PackedPolygons([{1: ring}], (30, 30))
    q = P.quantise(ring)
    want = [[*a, *b] for a, b in zip(q.tolist(), np.roll(q, -1, axis=0).tolist())]
    assert p.edge_xy.tolist() == [e for e in want if any(min(e[1], e[3]) <= 256 * y + 128 < max(e[1], e[3]) for y in range(30))]
    assert q[-2].tolist() == [256, 514] and q[-1].tolist() == [1794, 7680]                 # 256.5, 513.5, 1794.5, 7679.5: ties to even


def test_python_refusals():
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import labels_from_polygons
    tri = [(1, 1), (5, 1), (3, 4)]
    PP = polygons.PackedPolygons
    with pytest.raises(RmemError, match=r'frame 1, value 7: a flat ring of 7 numbers'):
        PP([{1: tri}, {7: [1, 1, 5, 1, 3, 4, 2]}], (8, 8))
    with pytest.raises(RmemError, match=r'frame 0, value 2: a ring of 2 vertices \(at least 3\)'):
        PP([{2: [(1, 1), (5, 1)]}], (8, 8))
    with pytest.raises(RmemError, match=r'frame 0, value 2: a ring of 2 vertices'):
        PP([{2: [tri, [1, 1, 5, 1]]}], (8, 8))
    for bad in (float('nan'), float('inf'), -float('inf'), 2.0 ** 20 + 1, -(2.0 ** 20) - 0.5):
        with pytest.raises(RmemError, match=r'frame 2, value 9: vertex .* is not finite or beyond 2\^20 pixels'):
            PP([{1: tri}, [], [(3, tri), (9, [tri, [(1, 1), (5, bad), (3, 4)]])]], (8, 8))
    PP([{1: [(-2.0 ** 20, 0), (2.0 ** 20, 1), (0, 2.0 ** 20)]}], (8, 8))               # the limit itself is accepted
    for value in (0, 256, -1, 1.5, 'a', None):
        with pytest.raises(RmemError, match=r'frame 0: label value .* outside 1\.\.255'):
            PP([[(value, tri)]], (8, 8))
    with pytest.raises(RmemError, match=r'frame 1 lists 256 shapes \(at most 255\)'):
        PP([[], [(1, tri)] * 256], (8, 8))
    PP([[(1, tri)] * 255], (8, 8))
    for frames, size in (([], (8, 8)), ([{}], (0, 8)), ([{}], (8, -1)), ([{}], (8193, 8192)), ([{}] * 65536, (1, 1))):
        with pytest.raises(RmemError, match=r'at least one frame, at most 65535, H \* W at most 2\^26'):
            PP(frames, size)
    with pytest.raises(RmemError, match=r'frame 0, value 1: size \[8, 9\] differs from the stack\'s \[8, 8\]'):
        PP([{1: {'size': [8, 9], 'segmentation': [[1, 1, 5, 1, 3, 4]]}}], (8, 8))
    with pytest.raises(RmemError, match=r'frame 0, value 1: a polygon dict has'):
        PP([{1: {'rings': [tri]}}], (8, 8))
    with pytest.raises(RmemError, match=r'frame 0, value 1: a shape is a ring, a list of rings'):
        PP([{1: 'triangle'}], (8, 8))
    with pytest.raises(RmemError, match=r'frame 0, value 1: a ring is an array-like \[k, 2\]'):
        PP([{1: [tri, [(1, 1, 1), (2, 2, 2), (3, 3, 3)]]}], (8, 8))
    with pytest.raises(RmemError, match=r'frame 0, value 1: a ring is an array-like \[k, 2\]'):
        PP([{1: [tri, ['a', 'b', 'c', 'd', 'e', 'f']]}], (8, 8))
    with pytest.raises(RmemError, match='256 tracks'):
        labels_from_polygons([{t: tri for t in range(256)}], (8, 8), 'cuda')           # refused before any device is touched
    with pytest.raises(RmemError, match='there is no host rasteriser'):
        polygons.fill_label_stack([{1: tri}], (8, 8), 'cpu')
    p = PP([{1: tri}], (8, 8))
    with pytest.raises(RmemError, match='packed must be a PackedPolygons'):
        polygons.fill_labels_into([{1: tri}], torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RmemError, match='out must be a uint8 device tensor'):
        polygons.fill_labels_into(p, torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RmemError, match='out must be a uint8 device tensor'):
        polygons.fill_labels_into(p, np.zeros((1, 8, 8), dtype=np.uint8))


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_workspace_budget_refusal_and_passes(lib):
    """passes() needs the library, not a GPU: whole frames per pass, the budget, and the refusal with the byte count"""
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    frames, H, W = _clip()
    p = polygons.PackedPolygons(frames + frames, (H, W))
    need = [int(lib.rmem_polygon_fill_workspace_bytes(int(w))) for w in p.frame_words]
    one = p.passes()
    assert len(one) == 1 and (one[0].frame0, one[0].frames, one[0].shape0, one[0].shapes) == (0, 6, 0, 14)
    assert (one[0].edge0, one[0].edges, one[0].cross0, one[0].crossings) == (0, p.nedges, 0, p.crossings)
    assert (one[0].plane0, one[0].plane_words) == (0, p.plane_words)
    each = p.passes(max(need))
    assert all(q.frames >= 1 for q in each) and [q.frame0 for q in each] == list(np.cumsum([0] + [q.frames for q in each[:-1]]))
    assert sum(q.frames for q in each) == 6 and sum(q.shapes for q in each) == 14 and sum(q.edges for q in each) == p.nedges
    assert sum(q.crossings for q in each) == p.crossings and sum(q.plane_words for q in each) == p.plane_words
    for q in each:
        assert int(lib.rmem_polygon_fill_workspace_bytes(q.plane_words)) <= max(need)
        assert q.cross0 == p.edge_first[q.edge0] and q.shape0 == p.frame_shape[q.frame0]
        assert q.plane_words == int(p.frame_words[q.frame0:q.frame0 + q.frames].sum())
        if q.shapes:
            assert q.plane0 == p.table['plane'][q.shape0]
    assert len(each) > 1
    for bad in (max(need) - 1, 0, 2.5, True, 'x'):
        with pytest.raises(RmemError, match=rf'workspace_bytes must be an integer of at least the largest frame\'s need, {max(need)} bytes'):
            p.passes(bad)


def test_workspace_query_is_the_planes_sum(lib):
    from rmem_ocu_amd import polygons
    Q = lib.rmem_polygon_fill_workspace_bytes
    assert Q(-1) == 0 and Q((1 << 34) + 1) == 0
    assert Q(0) == 16 and Q(1) == 16 and Q(4) == 16 and Q(5) == 32 and Q(1 << 34) == 4 << 34
    frames, H, W = _clip()
    p = polygons.PackedPolygons(frames, (H, W))
    words = sum((int(r['y1']) - int(r['y0'])) * ((int(r['x1']) - int(r['x0']) + 31) // 32) for r in p.table)
    assert words == p.plane_words > 0 and Q(p.plane_words) == (4 * words + 15) // 16 * 16
    full = polygons.PackedPolygons([{1: [(0, 0), (854, 0), (854, 480), (0, 480)]}], (480, 854))
    assert full.plane_words == 480 * 27 and full.crossings == 2 * 480 and full.nedges == 2


def test_c_refusals_need_no_gpu(lib):
    """every RMEM_REQUIRE of rmem_polygon_fill_labels, by message"""
    from rmem_ocu_amd import _lib
    A = 64                                                               # a non-null, 16-byte aligned address that is never used

    def call(xy=A, shape=A, first=A, nedges=4, table=A, nshapes=2, frame_shape=A, n=3, H=4, W=4, workspace=A, ws_bytes=64, labels=A,
             status=A, no_pass=False, **kw):
        fields = dict(frame0=0, frames=3, shape0=0, shapes=2, edge0=0, edges=4, cross0=0, crossings=9, plane0=0, plane_words=8)
        fields.update(kw)
        p = _lib.PolyPass(**fields)
        return lib.rmem_polygon_fill_labels(xy, shape, first, nedges, table, nshapes, frame_shape, n, H, W, None if no_pass else ctypes.byref(p),
                                            workspace, ws_bytes, labels, status, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.rmem_last_error_string(), (rc, lib.rmem_last_error_string())

    for name in ('xy', 'shape', 'first', 'table', 'frame_shape', 'workspace', 'labels', 'status'):
        refused(call(**{name: None}), b'null pointer')
    refused(call(no_pass=True), b'null pointer')
    refused(call(n=0), b'frames must be in 1..65535')
    refused(call(n=65536), b'frames must be in 1..65535')
    refused(call(H=0), b'H and W must be positive')
    refused(call(W=-1), b'H and W must be positive')
    refused(call(H=8193, W=8192), b'2^26')
    refused(call(nshapes=0), b'nshapes must be in 1..65535*255')
    refused(call(nshapes=65535 * 255 + 1), b'nshapes must be in 1..65535*255')
    refused(call(nedges=-1), b'nedges must be in 0..2^30')
    refused(call(nedges=(1 << 30) + 1), b'nedges must be in 0..2^30')
    refused(call(frame0=-1), b"the pass's frames")
    refused(call(frames=0), b"the pass's frames")
    refused(call(frame0=1, frames=3), b"the pass's frames")
    refused(call(shape0=-1), b"the pass's shapes")
    refused(call(shapes=-1), b"the pass's shapes")
    refused(call(shape0=1, shapes=2), b"the pass's shapes")
    refused(call(edge0=-1), b"the pass's edges")
    refused(call(edges=-1), b"the pass's edges")
    refused(call(edge0=3, edges=2), b"the pass's edges")
    refused(call(cross0=-1), b"the pass's crossings must lie in 0..2^31-1")
    refused(call(crossings=-1), b"the pass's crossings must lie in 0..2^31-1")
    refused(call(crossings=1 << 31), b"the pass's crossings must lie in 0..2^31-1")
    refused(call(cross0=1 << 30, crossings=1 << 30), b"the pass's crossings must lie in 0..2^31-1")
    refused(call(edges=0), b'crossings need edges and shapes')
    refused(call(shapes=0), b'crossings need edges and shapes')
    refused(call(plane0=-1), b"the pass's plane words")
    refused(call(plane_words=-1), b"the pass's plane words")
    refused(call(plane_words=(1 << 34) + 1), b"the pass's plane words")
    refused(call(workspace=A + 8), b'the workspace must be 16-byte aligned')
    refused(call(xy=A + 4), b'edge_xy must be 16-byte aligned')
    refused(call(ws_bytes=16), b'the workspace is smaller than')
    refused(call(plane_words=17, ws_bytes=64), b'the workspace is smaller than')


# ---------------------------------------------------------------------------------------------------------------- evaluator
def test_labels_from_polygons_id_mapping(monkeypatch):
    """the listing: ids -> values, tracks left out, the default ids; the fill is the restatement's painter"""
    from rmem_ocu_amd import evaluator, polygons
    H, W = 9, 11
    a, b, c = [(1, 1), (6, 1), (6, 5), (1, 5)], [(4, 3), (10, 3), (10, 8), (4, 8)], [(0, 6), (3, 6), (3, 9), (0, 9)]
    seen = {}

    def fake_fill(frames, size=None, device=None):
        seen['frames'], seen['size'], seen['device'] = frames, size, device
        return P.paint_stack([[(v, [s]) for v, s in fr] for fr in frames], *size)

    monkeypatch.setattr(polygons, 'fill_label_stack', fake_fill)
    frames = [{'dog': a, 'cat': b}, {'cat': b}, {'eel': c, 'dog': a}]
    labels, ids = evaluator.labels_from_polygons(frames, (H, W), 'cuda:0')
    assert ids == ['cat', 'dog', 'eel'] and seen['size'] == (H, W) and seen['device'] == 'cuda:0'
    assert seen['frames'] == [[(2, a), (1, b)], [(1, b)], [(3, c), (2, a)]]               # listing order is the frame's own
    assert np.array_equal(labels, P.paint_stack([[(2, [a]), (1, [b])], [(1, [b])], [(3, [c]), (2, [a])]], H, W))
    assert labels[0, 4, 5] == 1 and labels[2, 4, 5] == 2                                 # the later listed wins where two overlap
    labels, ids = evaluator.labels_from_polygons(frames, (H, W), 'cuda:0', ids=['eel', 'dog'])
    assert ids == ['eel', 'dog'] and seen['frames'] == [[(2, a)], [], [(1, c), (2, a)]]    # 'cat' is left out
    _, ids = evaluator.labels_from_polygons([{5: a}, {2: b}], (H, W), 'cuda:0')
    assert ids == [2, 5]


def test_product_does_not_import_the_reference():
    for dp, _, files in os.walk(os.path.join(ROOT, 'rmem_ocu_amd')):
        for f in files:
            if f.endswith('.py'):
                assert not re.search(r'polyfill_ref|polygons_ref', open(os.path.join(dp, f)).read()), f
