"""The stroke rasteriser without a GPU: the restatement of the contract (tests/strokes_ref.py) on hand cases and seeded properties,
its agreement with a float64 distance test, the host pack of rmem_ocu_amd/strokes.py against a direct count, every refusal by
message, the workspace query, the passes, and the three evaluator wrappers with the draw stubbed by the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import strokes_ref as S
from conftest import ROOT


def _px(stroke, H, W):
    value, path, radius = S.stroke_parts(stroke)
    return S.stroke_pixels(path, radius, H, W)


# ---------------------------------------------------------------------------------------------------------------- hand cases
def test_a_dot():
    assert _px((1, [(3, 2)], 0), 5, 6) == {(2, 3)}
    assert _px((1, [(3, 2)], 1.5), 5, 6) == {(y, x) for y in range(5) for x in range(6) if (x - 3) ** 2 + (y - 2) ** 2 <= 2.25}
    assert len(_px((1, [(3, 2)], 1.5), 5, 6)) == 9
    assert _px((1, [(3.4, 1.6)], 0), 5, 6) == {(2, 3)}


def test_axis_aligned_and_diagonal_segments():
    assert _px((1, [(1, 2), (4, 2)], 0), 5, 6) == {(2, 1), (2, 2), (2, 3), (2, 4)}
    assert _px((1, [(2, 4), (2, 0)], 0), 5, 6) == {(y, 2) for y in range(5)}
    assert _px((1, [(0, 0), (4, 4)], 0), 5, 6) == {(i, i) for i in range(5)}
    assert _px((1, [(4, 0), (0, 4)], 0), 5, 6) == {(i, 4 - i) for i in range(5)}
    assert _px((1, [(1, 2), (4, 2)], 1), 5, 6) == {(2, x) for x in range(6)} | {(1, x) for x in range(1, 5)} | {(3, x) for x in range(1, 5)}
    diag = _px((1, [(0, 0), (4, 4)], 0.75), 5, 6)                       # |x - y| / sqrt 2 <= 0.75: the diagonal and its two neighbours
    assert diag == {(y, x) for y in range(5) for x in range(6) if abs(x - y) <= 1 and x <= 4}   # (4, 5) is 1 from the end


@pytest.mark.parametrize('case', S.tie_cases(), ids=lambda c: c[0])
def test_ties_and_vertices_on_centres_and_corners(case):
    name, stroke, H, W, want = case
    assert _px(stroke, H, W) == want, name


def test_a_short_segment_between_two_sample_columns_draws_its_endpoints():
    assert _px((1, [(2.2, 1.1), (2.7, 1.3)], 0), 4, 5) == {(1, 2), (1, 3)}       # no integer k inside: the endpoints alone
    assert _px((1, [(2.2, 1.1), (2.4, 1.3)], 0), 4, 5) == {(1, 2)}


def test_a_zero_length_segment_inside_a_polyline_changes_nothing():
    for r in (0, 1.25):
        assert _px((1, [(1, 1), (3, 2), (3, 2), (3.0004, 2), (5, 0)], r), 4, 7) == _px((1, [(1, 1), (3, 2), (5, 0)], r), 4, 7)
    assert S.points([(1, 1), (1, 1), (1.001, 1)]) == [(256, 256)]


def test_a_stroke_off_the_frame_draws_nothing_and_is_no_error():
    for r in (0, 2):
        assert _px((1, [(-9, -9), (-4, -3)], r), 5, 5) == set()
        assert _px((1, [(9, 1), (30, 2)], r), 5, 5) == set()
    assert _px((1, [(-3, 2), (8, 2)], 0), 5, 5) == {(2, x) for x in range(5)}   # clipped, not dropped


def test_an_eraser_over_an_earlier_stroke_and_over_a_base():
    frames = [[(7, [(0, 1), (5, 1)], 0), (0, [(2, 0), (2, 3)], 0), (9, [(4, 1)], 0)]]
    got = S.paint_stack(frames, 3, 6)
    assert got[0, 1].tolist() == [7, 7, 0, 7, 9, 7] and not got[0, 0].any() and not got[0, 2].any()
    base = np.full((1, 3, 6), 5, dtype=np.uint8)
    over = S.paint_stack(frames, 3, 6, base)
    assert over[0, 1].tolist() == [7, 7, 0, 7, 9, 7] and over[0, 0].tolist() == [5, 5, 0, 5, 5, 5] and (base == 5).all()


# ---------------------------------------------------------------------------------------------------------------- properties
def test_a_reversed_polyline_gives_identical_pixels():
    rng = np.random.default_rng(5)
    for i in range(40):
        H, W = int(rng.integers(1, 20)), int(rng.integers(1, 30))
        path = S.random_walk(rng, H, W, int(rng.integers(1, 6)), margin=2.0)
        for r in (0, 0.4, 1, 2.5):
            assert S.stroke_pixels(path, r, H, W) == S.stroke_pixels(path[::-1], r, H, W), (i, r)


def test_every_hairline_inside_the_frame_is_one_8_connected_piece():
    rng = np.random.default_rng(6)
    for i in range(60):
        H, W = int(rng.integers(2, 40)), int(rng.integers(2, 40))
        path = np.clip(S.random_walk(rng, H, W, int(rng.integers(1, 7))), 0, (W - 1, H - 1))
        px = S.stroke_pixels(path, 0, H, W)
        assert px and S.components8(px) == 1, (i, path)


def test_radii_nest():
    rng = np.random.default_rng(7)
    for i in range(20):
        H, W = 17, 23
        path = S.random_walk(rng, H, W, 4, margin=2.0)
        sets = [S.stroke_pixels(path, r, H, W) for r in (1 / 256, 0.4, 1, 1.004, 2.5, 7)]
        assert all(a <= b for a, b in zip(sets, sets[1:])), i
        assert {(y, x) for y, x in S.stroke_pixels(np.rint(path), 0, H, W)} <= S.stroke_pixels(np.rint(path), 0.75, H, W)


def test_a_dot_at_a_pixel_with_an_integer_radius_is_the_exact_disc():
    for (cx, cy, r) in ((10, 9, 1), (10, 9, 5), (0, 0, 7), (20, 3, 13), (4, 18, 25)):
        want = {(y, x) for y in range(21) for x in range(24) if (x - cx) ** 2 + (y - cy) ** 2 <= r * r}
        assert _px((1, [(cx, cy)], r), 21, 24) == want


def test_a_path_of_8_neighbour_pixels_draws_exactly_itself():
    rng = np.random.default_rng(8)
    for i in range(40):
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        path = S.neighbour_path(rng, H, W, int(rng.integers(1, 60)))
        assert S.stroke_pixels(path, 0, H, W) == {(y, x) for x, y in path}, i


def test_the_array_form_of_the_brush_rule_is_the_rule():
    rng = np.random.default_rng(9)
    for i in range(30):
        H, W = int(rng.integers(1, 20)), int(rng.integers(1, 30))
        pts = S.points(S.random_walk(rng, H, W, int(rng.integers(1, 5)), margin=2.0))
        R = int(rng.integers(1, 2000))
        assert np.array_equal(S.brush_mask_large(pts, R, H, W), S.mask_of(S.brush_pixels(pts, R, H, W), H, W)), i
    far = [(-(2 ** 28), 2 ** 28), (2 ** 28, -(2 ** 28))]                # the largest terms the contract allows
    assert np.array_equal(S.brush_mask_large(far, 65536, 9, 9), S.mask_of(S.brush_pixels(far, 65536, 9, 9), 9, 9))


def test_agreement_with_a_float_distance_test():
    """100 round-brush strokes on the 1/256 grid, where float64 sees exactly what the quantiser sees: every pixel of the frame
    whose float distance differs from r by more than 1e-6 must agree; the cap on what that leaves out is asserted"""
    rng = np.random.default_rng(2024)
    H, W = 24, 31
    checked = skipped = 0
    for i in range(100):
        path = S.random_walk(rng, H, W, 1 + i % 5, margin=3.0, grid=1 / 256)
        r = int(rng.integers(1, 8 * 256)) / 256
        dist = S.float_distance(path, H, W)
        got = S.mask_of(S.stroke_pixels(path, r, H, W), H, W)
        sure = np.abs(dist - r) > 1e-6
        assert np.array_equal(got[sure], (dist <= r)[sure]), (i, np.argwhere(sure & (got != (dist <= r)))[:4])
        checked += int(sure.sum())
        skipped += int((~sure).sum())
    assert skipped <= 0.005 * (checked + skipped), (skipped, checked)


# ---------------------------------------------------------------------------------------------------------------- the pack
def _direct(frames, H, W):
    """the tables of a pack, counted stroke by stroke in Python integers"""
    seg_xy, seg_stroke, counts, table, frame_stroke = [], [], [], [], [0]
    for f, strokes in enumerate(frames):
        for st in strokes:
            value, path, radius = S.stroke_parts(st)
            R, s = S.quantise(radius), len(table)
            box = None
            for A, B in S.segments(S.points(path)):
                if R == 0:
                    M = 0 if abs(B[0] - A[0]) >= abs(B[1] - A[1]) else 1
                    if B[M] < A[M]:
                        A, B = B, A
                    lo = [(min(A[i], B[i]) + 128) >> 8 for i in (0, 1)]
                    hi = [(max(A[i], B[i]) + 128) >> 8 for i in (0, 1)]
                else:
                    lo = [-((R - min(A[i], B[i])) // 256) for i in (0, 1)]
                    hi = [(max(A[i], B[i]) + R) // 256 for i in (0, 1)]
                x0, y0, x1, y1 = max(lo[0], 0), max(lo[1], 0), min(hi[0] + 1, W), min(hi[1] + 1, H)
                if x0 >= x1 or y0 >= y1:
                    continue
                if R == 0:
                    ks = [k for k in range((W, H)[M]) if A[M] <= 256 * k <= B[M]] if A != B else []
                    n = 2 + len(ks)
                else:
                    n = y1 - y0
                seg_xy.append([A[0], A[1], B[0], B[1]])
                seg_stroke.append(s)
                counts.append(n)
                box = (x0, y0, x1, y1) if box is None else (min(box[0], x0), min(box[1], y0), max(box[2], x1), max(box[3], y1))
            table.append((f, value, R) + (box or (0, 0, 0, 0)))
        frame_stroke.append(len(table))
    stroked = [f for f in range(len(frames)) if frame_stroke[f] < frame_stroke[f + 1]]
    return seg_xy, seg_stroke, [0] + list(np.cumsum(counts)), table, frame_stroke, stroked


def _clip(H=19, W=33):
    return [S.random_strokes(11, H, W, 4), [], S.random_strokes(12, H, W, 9), [{'value': 3, 'path': [(-40, -40)], 'radius': 2}],
            S.random_strokes(13, H, W, 2)], H, W


def test_packed_layout_against_a_direct_count():
    from rmem_ocu_amd import strokes
    frames, H, W = _clip()
    p = strokes.PackedStrokes(frames, (H, W))
    xy, ss, first, table, fs, stroked = _direct(frames, H, W)
    assert p.nstrokes == len(table) == 16 and len(p) == 16 and p.nsegs == len(xy) and p.items == first[-1] > 0
    assert p.seg_xy.tolist() == xy and p.seg_stroke.tolist() == ss and p.seg_first.tolist() == first
    assert p.frame_stroke.tolist() == fs and p.stroked.tolist() == stroked == [0, 2, 3, 4]
    for k, row in enumerate(table):
        got = p.table[k]
        assert tuple(int(got[n]) for n in ('frame', 'value', 'radius', 'x0', 'y0', 'x1', 'y1')) == row, k
        assert stroked[int(got['slot'])] == row[0]
    assert p.table[13]['x1'] == 0 and p.stroke_seg[13] == p.stroke_seg[14]          # the stroke off the frame has no segment
    E, n = p.nsegs, 5
    ints = p.buf.numpy().view(np.int32)
    assert p.offsets == (0, 16 * E, 20 * E, 24 * E + 4, 24 * E + 4 + 4 * (n + 1)) and ints.size == 6 * E + 1 + n + 1 + 4
    assert ints[:4 * E].reshape(E, 4).tolist() == xy and ints[4 * E:5 * E].tolist() == ss and ints[5 * E:6 * E + 1].tolist() == first
    assert ints[6 * E + 1:6 * E + 2 + n].tolist() == fs and ints[6 * E + 2 + n:].tolist() == stroked
    assert strokes.STROKE_DTYPE.itemsize == 32 == ctypes.sizeof(__import__('rmem_ocu_amd._lib', fromlist=['Stroke']).Stroke)
    assert p.desc_bytes.numpy().view(strokes.STROKE_DTYPE).tolist() == p.table.tolist()
    hair = strokes.PackedStrokes([[(1, [(5, 1), (1, 2)], 0), (2, [(1, 5), (2, 1)], 0)]], (8, 8))
    assert hair.seg_xy.tolist() == [[256, 512, 1280, 256], [512, 256, 256, 1280]] and hair.seg_first.tolist() == [0, 7, 14]


def test_every_stroke_form_packs_to_identical_bytes():
    from rmem_ocu_amd import strokes
    H, W = 12, 17
    path = [[1.5, 2.25], [7, 3], [7, 3], [16.5, 11]]
    forms = [{'value': 4, 'path': path, 'radius': 1.5}, (4, path, 1.5), [4, np.array(path), 1.5], {'value': np.uint8(4), 'path': [c for p in path for c in p], 'radius': 1.5},
             (4.0, tuple(map(tuple, path)), np.float32(1.5))]
    packs = [strokes.PackedStrokes([[f], []], (H, W)) for f in forms]
    for q in packs[1:]:
        assert q.buf.numpy().tobytes() == packs[0].buf.numpy().tobytes() and q.desc_bytes.numpy().tobytes() == packs[0].desc_bytes.numpy().tobytes()
    a = strokes.PackedStrokes([[{'value': 4, 'path': path}]], (H, W))
    b = strokes.PackedStrokes([[(4, path)]], (H, W))
    c = strokes.PackedStrokes([[(4, path, 0)]], (H, W))
    assert a.buf.numpy().tobytes() == b.buf.numpy().tobytes() == c.buf.numpy().tobytes() and int(a.table[0]['radius']) == 0
    corner = strokes.PackedStrokes([[(4, [[x + 0.5, y + 0.5] for x, y in path], 1.5)]], (H, W), origin='corner')
    centre = strokes.PackedStrokes([[(4, path, 1.5)]], (H, W))
    assert corner.buf.numpy().tobytes() == centre.buf.numpy().tobytes()
    assert np.array_equal(S.paint_stack([[(4, [[x + 0.5, y + 0.5] for x, y in path], 1.5)]], H, W, origin='corner'), S.paint_stack([[(4, path, 1.5)]], H, W))


def test_packing_quantises_like_the_reference():
    from rmem_ocu_amd import strokes
    xs = [0.001953125, 0.005859375, 1.498046875, -2.501953125, 3.3, 1e-9, 1048576.0, -1048576.0]      # ties to even among them
    p = strokes.PackedStrokes([[(1, [(x, 0.0), (x + 300, 0)], 0)] for x in xs[:6]], (4, 4))
    assert p.seg_xy[:, 0].tolist() == [S.quantise(x) for x in xs[:6]] == [0, 2, 384, -640, 845, 0]
    strokes.PackedStrokes([[(1, [(xs[6], xs[7])], 0)]], (4, 4))
    assert int(strokes.PackedStrokes([[(1, [(0, 0)], 0.001953125)]], (4, 4)).table[0]['radius']) == 0
    assert int(strokes.PackedStrokes([[(1, [(0, 0)], 256)]], (4, 4)).table[0]['radius']) == 65536


def test_python_refusals():
    from rmem_ocu_amd import strokes
    from rmem_ocu_amd._lib import RmemError
    P = strokes.PackedStrokes
    ok = (1, [(1, 1)], 0)
    for frames, size, text in (([], (4, 4), '0 frames of 4x4'), ([[ok]], (0, 4), '1 frames of 0x4'), ([[ok]], (8193, 8192), 'H \\* W at most 2\\^26'),
                               ([{1: ok}], (4, 4), 'frame 0 must be a list of strokes \\(got dict\\)'),
                               ([[ok], 7], (4, 4), 'frame 1 must be a list of strokes \\(got int\\)'),
                               ([[ok, 5]], (4, 4), 'frame 0, stroke 1: a stroke is a dict'),
                               ([[{'value': 1}]], (4, 4), 'frame 0, stroke 0: a stroke dict has \'value\', \'path\''),
                               ([[(256, [(1, 1)])]], (4, 4), 'value 256 outside 0..255'), ([[(-1, [(1, 1)])]], (4, 4), 'value -1 outside 0..255'),
                               ([[(1.5, [(1, 1)])]], (4, 4), 'value 1.5 outside 0..255'), ([[(True, [(1, 1)])]], (4, 4), 'value True outside'),
                               ([[(1, [(1, 1)], -0.5)]], (4, 4), 'radius must be a finite number in 0..256 pixels \\(got -0.5\\)'),
                               ([[(1, [(1, 1)], 256.5)]], (4, 4), 'radius must be a finite number'), ([[(1, [(1, 1)], float('nan'))]], (4, 4), 'radius must be'),
                               ([[(1, [(1, 1)], '2')]], (4, 4), 'radius must be'),
                               ([[(1, [1, 2, 3])]], (4, 4), 'a flat path of 3 numbers'), ([[(1, [])]], (4, 4), 'a path without a point'),
                               ([[(1, [[1, 2, 3]])]], (4, 4), 'a path is an array-like \\[k, 2\\]'), ([[(1, 'abc')]], (4, 4), 'a path is an array-like'),
                               ([[ok], [(9, [(1, float('inf'))])]], (4, 4), 'frame 1, value 9: point \\(1.0, inf\\) is not finite or beyond'),
                               ([[(2, [(1, 1), (float('nan'), 1)])]], (4, 4), 'frame 0, value 2: point \\(nan, 1.0\\)'),
                               ([[(2, [(1048576.5, 1)])]], (4, 4), 'beyond 2\\^20 pixels')):
        with pytest.raises(RmemError, match='PackedStrokes: .*' + text):
            P(frames, size)
    with pytest.raises(RmemError, match='origin must be \'centre\' or \'corner\''):
        P([[ok]], (4, 4), origin='center')
    p = P([[ok]], (8, 8))
    with pytest.raises(RmemError, match='packed must be a PackedStrokes'):
        strokes.draw_labels_into([[ok]], torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RmemError, match='out must be a uint8 device tensor'):
        strokes.draw_labels_into(p, torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RmemError, match='out must be a uint8 device tensor'):
        strokes.draw_labels_into(p, np.zeros((1, 8, 8), dtype=np.uint8))
    with pytest.raises(RmemError, match='the target must be a GPU device'):
        strokes.draw_label_stack([[ok]], (8, 8), 'cpu')


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_workspace_query(lib):
    Q = lib.rmem_stroke_workspace_bytes
    assert Q(-1, 4, 4) == 0 and Q(65536, 4, 4) == 0 and Q(1, 0, 4) == 0 and Q(1, 4, -1) == 0 and Q(1, 8193, 8192) == 0
    assert Q(0, 4, 4) == 16 and Q(1, 1, 1) == 16 and Q(1, 1, 5) == 32 and Q(3, 19, 33) == (3 * 19 * 33 * 4 + 15) // 16 * 16
    assert Q(64, 480, 854) == 64 * 480 * 854 * 4 and Q(65535, 8192, 8192) == 65535 * (1 << 26) * 4


def test_passes_and_the_workspace_budget(lib):
    """passes() needs the library, not a GPU: whole frames per pass, owner maps for the stroked frames only"""
    from rmem_ocu_amd import strokes
    from rmem_ocu_amd._lib import RmemError
    frames, H, W = _clip()
    p = strokes.PackedStrokes(frames + frames, (H, W))
    one_map = int(lib.rmem_stroke_workspace_bytes(1, H, W))
    one = p.passes()
    assert len(one) == 1 and (one[0].frame0, one[0].frames, one[0].stroke0, one[0].strokes) == (0, 10, 0, 32)
    assert (one[0].seg0, one[0].segs, one[0].slot0, one[0].slots, one[0].item0, one[0].items) == (0, p.nsegs, 0, 8, 0, p.items)
    each = p.passes(one_map)
    assert [(q.frame0, q.frames, q.slots) for q in each] == [(0, 2, 1), (2, 1, 1), (3, 1, 1), (4, 1, 1), (5, 2, 1), (7, 1, 1), (8, 1, 1), (9, 1, 1)]
    pairs = p.passes(2 * one_map)
    assert [(q.frame0, q.frames, q.slots) for q in pairs] == [(0, 3, 2), (3, 2, 2), (5, 3, 2), (8, 2, 2)]
    for plan in (each, pairs):
        assert sum(q.strokes for q in plan) == 32 and sum(q.segs for q in plan) == p.nsegs and sum(q.items for q in plan) == p.items
        for q in plan:
            assert q.stroke0 == p.frame_stroke[q.frame0] and q.seg0 == p.stroke_seg[q.stroke0] and q.item0 == p.seg_first[q.seg0]
            assert p.stroked[q.slot0:q.slot0 + q.slots].tolist() == [f for f in range(q.frame0, q.frame0 + q.frames) if f % 5 != 1]
    for bad in (one_map - 1, 0, 2.5, True, 'x'):
        with pytest.raises(RmemError, match=rf'workspace_bytes must be an integer of at least one frame\'s need, {one_map} bytes'):
            p.passes(bad)
    empty = strokes.PackedStrokes([[], []], (H, W))
    q = empty.passes()
    assert len(q) == 1 and (q[0].frames, q[0].strokes, q[0].slots, q[0].items) == (2, 0, 0, 0) and len(empty) == 0


def test_c_refusals_need_no_gpu(lib):
    """every RMEM_REQUIRE of rmem_stroke_draw_labels, by message"""
    from rmem_ocu_amd import _lib
    A = 64                                                               # a non-null, 16-byte aligned address that is never used

    def call(xy=A, stroke=A, first=A, nsegs=4, table=A, nstrokes=2, frame_stroke=A, stroked=A, nstroked=2, n=3, H=4, W=4, workspace=A,
             ws_bytes=128, labels=A, status=A, no_pass=False, **kw):
        fields = dict(frame0=0, frames=3, stroke0=0, strokes=2, seg0=0, segs=4, slot0=0, slots=2, item0=0, items=9)
        fields.update(kw)
        p = _lib.StrokePass(**fields)
        return lib.rmem_stroke_draw_labels(xy, stroke, first, nsegs, table, nstrokes, frame_stroke, stroked, nstroked, n, H, W,
                                           None if no_pass else ctypes.byref(p), workspace, ws_bytes, labels, 0, status, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.rmem_last_error_string(), (rc, lib.rmem_last_error_string())

    for name in ('xy', 'stroke', 'first', 'table', 'frame_stroke', 'stroked', 'workspace', 'labels', 'status'):
        refused(call(**{name: None}), b'null pointer')
    refused(call(no_pass=True), b'null pointer')
    refused(call(n=0), b'frames must be in 1..65535')
    refused(call(n=65536), b'frames must be in 1..65535')
    refused(call(H=0), b'H and W must be positive')
    refused(call(W=-1), b'H and W must be positive')
    refused(call(H=8193, W=8192), b'2^26')
    refused(call(nstrokes=0), b'nstrokes must be in 1..2^30')
    refused(call(nstrokes=(1 << 30) + 1), b'nstrokes must be in 1..2^30')
    refused(call(nsegs=-1), b'nsegs must be in 0..2^30')
    refused(call(nsegs=(1 << 30) + 1), b'nsegs must be in 0..2^30')
    refused(call(nstroked=0), b'nstroked must be in 1..frames')
    refused(call(nstroked=4), b'nstroked must be in 1..frames')
    refused(call(frame0=-1), b"the pass's frames")
    refused(call(frames=0), b"the pass's frames")
    refused(call(frame0=1, frames=3), b"the pass's frames")
    refused(call(stroke0=-1), b"the pass's strokes")
    refused(call(strokes=-1), b"the pass's strokes")
    refused(call(stroke0=1, strokes=2), b"the pass's strokes")
    refused(call(seg0=-1), b"the pass's segments")
    refused(call(segs=-1), b"the pass's segments")
    refused(call(seg0=3, segs=2), b"the pass's segments")
    refused(call(slot0=-1), b"the pass's slots")
    refused(call(slots=-1), b"the pass's slots")
    refused(call(slot0=1, slots=2), b"the pass's slots")
    refused(call(frame0=2, frames=1, slots=2), b"the pass's slots")
    refused(call(item0=-1), b"the pass's items must lie in 0..2^31-1")
    refused(call(items=-1), b"the pass's items must lie in 0..2^31-1")
    refused(call(items=1 << 31), b"the pass's items must lie in 0..2^31-1")
    refused(call(item0=1 << 30, items=1 << 30), b"the pass's items must lie in 0..2^31-1")
    refused(call(segs=0), b'items need segments and strokes')
    refused(call(strokes=0), b'items need segments and strokes')
    refused(call(slots=0), b'strokes need a slot')
    refused(call(workspace=A + 8), b'the workspace must be 16-byte aligned')
    refused(call(xy=A + 4), b'seg_xy must be 16-byte aligned')
    refused(call(ws_bytes=112), b'the workspace is smaller than')
    refused(call(H=5, ws_bytes=128), b'the workspace is smaller than')


# ---------------------------------------------------------------------------------------------------------------- evaluator
@pytest.fixture
def stub(monkeypatch):
    """strokes.draw_label_stack replaced by the restatement's painter; what it was given is kept"""
    from rmem_ocu_amd import strokes
    seen = {}

    def fake(frames, size=None, device=None, base=None):
        seen['frames'], seen['size'], seen['device'] = frames, size, device
        return S.paint_stack(frames, *size)

    monkeypatch.setattr(strokes, 'draw_label_stack', fake)
    return seen


def test_seeds_from_scribbles(stub):
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    yx = lambda *p: np.array(p, dtype=np.int32)
    scribbles = [{2: {'positive': True, 'path': yx((1, 1), (2, 2), (3, 2)), 'depth2': 9}, 1: {'positive': False, 'path': yx((2, 0), (2, 1), (2, 2)), 'depth2': 4}},
                 {}, {3: {'positive': True, 'path': yx((0, 5)), 'depth2': 4}}]
    got = evaluator.seeds_from_scribbles(scribbles, (5, 7), 'cuda:0', background=9)
    assert stub['size'] == (5, 7) and stub['device'] == 'cuda:0' and [len(f) for f in stub['frames']] == [2, 0, 1]
    assert [s['value'] for s in stub['frames'][0]] == [9, 2]                              # ascending object id: 1 (negative), then 2
    want = np.zeros((3, 5, 7), dtype=np.uint8)
    want[0, 2, 0] = want[0, 2, 1] = 9
    want[0, 1, 1] = want[0, 2, 2] = want[0, 3, 2] = 2                                     # (y, x) swapped for the caller; object 2 wins at (2, 2)
    want[2, 0, 5] = 3
    assert np.array_equal(got, want)
    wide = evaluator.seeds_from_scribbles(scribbles, (5, 7), 'cuda:0', radius=1, background=9)
    assert all(s['radius'] == 1 for f in stub['frames'] for s in f) and wide[2, 1, 5] == 3 and wide[2, 0, 4] == 3
    with pytest.raises(RmemError, match='object 1 has a negative seed: give background'):
        evaluator.seeds_from_scribbles(scribbles, (5, 7), 'cuda:0')
    with pytest.raises(RmemError, match='background must be None or an integer in 1..255'):
        evaluator.seeds_from_scribbles(scribbles, (5, 7), 'cuda:0', background=0)


def test_seeds_from_clicks(stub):
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    clicks = np.array([[(1, 2, 1, 4), (-1, -1, 0, 0), (3, 0, 0, 1)], [(-1, -1, 0, 0)] * 3], dtype=np.int32)
    got = evaluator.seeds_from_clicks(clicks, (4, 5), 'cuda:0', background=200)
    want = np.zeros((2, 4, 5), dtype=np.uint8)
    want[0, 1, 2], want[0, 3, 0] = 1, 200
    assert np.array_equal(got, want) and [len(f) for f in stub['frames']] == [2, 0]
    disc = evaluator.seeds_from_clicks(clicks, (4, 5), 'cuda:0', radius=1, background=200)
    assert disc[0, 0, 2] == disc[0, 1, 1] == disc[0, 1, 3] == disc[0, 2, 2] == 1 and disc[0, 0, 1] == 0
    with pytest.raises(RmemError, match='object 3 has a negative seed'):
        evaluator.seeds_from_clicks(clicks, (4, 5), 'cuda:0')
    for bad in (clicks[0], clicks.astype(np.float32), clicks[:, :, :3]):
        with pytest.raises(RmemError, match=r'clicks must be an integer array \[n, num_objs, 4\]'):
            evaluator.seeds_from_clicks(bad, (4, 5), 'cuda:0')


def test_labels_from_scribbles(stub):
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    H, W = 5, 9
    doc = {'scribbles': [[{'path': [[0.0, 0.0], [0.49, 0.3], [1.0, 1.0]], 'object_id': 2, 'start_time': 0},
                          {'path': [[0.5, 0.5]], 'object_id': 7}], [], [{'path': [], 'object_id': 1}]], 'sequence': 'x'}
    got = evaluator.labels_from_scribbles(doc, (H, W), 'cuda:0')
    assert stub['frames'][0][0]['path'].tolist() == [[0, 0], [3, 1], [8, 4]] and stub['frames'][0][1]['path'].tolist() == [[4, 2]]
    assert [len(f) for f in stub['frames']] == [2, 0, 0] and got.shape == (3, H, W) and got.dtype == np.uint8
    assert got[0, 0, 0] == 2 and got[0, 1, 3] == 2 and got[0, 4, 8] == 2 and got[0, 2, 4] == 7 and set(np.unique(got)) == {0, 2, 7}
    only = evaluator.labels_from_scribbles(doc, (H, W), 'cuda:0', ids=[7, 5])
    assert [len(f) for f in stub['frames']] == [1, 0, 0] and only[0, 2, 4] == 1 and set(np.unique(only)) == {0, 1}
    with pytest.raises(RmemError, match='path coordinates must lie in \\[0, 1\\]'):
        evaluator.labels_from_scribbles({'scribbles': [[{'path': [[0.5, 1.01]], 'object_id': 1}]]}, (H, W), 'cuda:0')
    with pytest.raises(RmemError, match='a scribble is a dict with \'path\' and \'object_id\''):
        evaluator.labels_from_scribbles({'scribbles': [[{'path': [[0.5, 0.5]]}]]}, (H, W), 'cuda:0')
    with pytest.raises(RmemError, match='doc must be a dict'):
        evaluator.labels_from_scribbles([[]], (H, W), 'cuda:0')


def test_product_does_not_import_the_reference():
    for dp, _, files in os.walk(os.path.join(ROOT, 'rmem_ocu_amd')):
        for f in files:
            if f.endswith('.py'):
                assert not re.search(r'strokes_ref', open(os.path.join(dp, f)).read()), f
