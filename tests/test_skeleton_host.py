"""What the thinning of label stacks rests on, checked without a GPU: the two tables (the library's export against the rule's
restatement), hand-written cases, the invariants of the operator on random small stacks, the tile argument, the longest path, the
scribble rule, workspace sizes and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

import skeleton_ref as R


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    return _lib.lib()


def _random_stack(rng):
    n, H, W = int(rng.integers(1, 3)), int(rng.integers(1, 13)), int(rng.integers(1, 17))
    values = int(rng.integers(1, 4))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return R.blobs(int(rng.integers(0, 1 << 30)), n, H, W, values=values, count=4)
    if kind == 1:
        return rng.integers(0, values + 1, (n, H, W)).astype(np.uint8)
    small = rng.integers(0, values + 1, (n, (H + 2) // 3, (W + 2) // 3)).astype(np.uint8)       # 3 x 3-blocky content
    return np.ascontiguousarray(np.repeat(np.repeat(small, 3, axis=1), 3, axis=2)[:, :H, :W])


def test_table_figures():
    t = R.tables()
    assert t.shape == (2, 256)
    assert int(t[0].sum()) == 37 and int(t[1].sum()) == 37
    assert int((t[0] & t[1]).sum()) == 6 and int((t[0] | t[1]).sum()) == 68
    assert np.nonzero(t[0])[0][:6].tolist() == [14, 20, 22, 28, 30, 52]
    assert np.nonzero(t[1])[0][:6].tolist() == [5, 7, 13, 14, 15, 28]


def test_exported_tables_equal_the_reference(lib):
    from rmem_ocu_amd import skeleton
    t = R.tables()
    for parity in (0, 1):
        buf = (ctypes.c_ubyte * 32)()
        assert lib.rmem_label_thin_table(parity, buf) == 0
        bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder='little').astype(bool)
        assert np.array_equal(bits, t[parity])
        got = skeleton.table(parity)
        assert got.dtype == bool and got.shape == (256,) and np.array_equal(got, t[parity])
        assert int(got.sum()) == 37
    th, tw, k = skeleton.tile()
    assert th >= 1 and tw >= 1 and k >= 2 and k % 2 == 0


def test_hand_cases():
    sq = np.zeros((4, 4), dtype=np.uint8)
    sq[1:3, 1:3] = 1
    want = np.zeros_like(sq)
    want[2, 1] = 1                                                   # a 2 x 2 square leaves its lower-left pixel
    assert np.array_equal(R.thin(sq), want)
    line = np.full((1, 17), 7, dtype=np.uint8)
    assert np.array_equal(R.thin(line), line)
    bar = np.full((2, 9), 255, dtype=np.uint8)
    want = np.zeros_like(bar)
    want[1, :8] = 255                                                # the first 8 pixels of the lower row
    assert np.array_equal(R.thin(bar), want)
    # a full 3 x 4 frame.  Even sub-iteration: the corner (0, 0) sees E, S, SE: X_H = 1 (x5 = 0 with x7), n1 = n2 = 2, and
    # (x2 | x3 | !x8) & x1 = 0, so it goes; so do the rest of the top row and the right column ((1, 3) sees N, NW, W, SW, S: X_H = 1,
    # n1 = n2 = 3, x1 = 0).  (1, 1) and (1, 2) see all eight neighbours, X_H = 0; (1, 0) and the bottom row have x1 = 1 with x2 or
    # x3 set, or fail G1, and stay.  Odd sub-iteration on the 2 x 3 rest: everything but (1, 1) and (1, 2) goes.
    full = np.ones((3, 4), dtype=np.uint8)
    s0, lost0 = R.sub_iteration(full, 0)
    assert s0.tolist() == [[0, 0, 0, 0], [1, 1, 1, 0], [1, 1, 1, 0]] and lost0.tolist() == [6]
    s1, lost1 = R.sub_iteration(s0, 1)
    assert s1.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]] and lost1.tolist() == [4]
    assert np.array_equal(R.thin(full), s1) and R.thin(full, with_iterations=True)[1] == 2
    out, lost = R.run(full, 0, 2)
    assert lost.tolist() == [[10, 10]] and R.run(full, 0, 3)[1].tolist() == [[10, 4]] and R.run(full, 1, 1)[1].tolist() == [[6, 6]]   # odd: the even rule turned by 180 degrees
    y, x = np.mgrid[0:21, 0:21]
    for r in (1, 4, 9):                                              # a disk of radius r takes r + 1 iterations
        assert R.thin(((y - 10) ** 2 + (x - 10) ** 2 <= r * r).astype(np.uint8), with_iterations=True)[1] == r + 1


def test_invariants_on_random_small_stacks():
    rng = np.random.default_rng(20261020)
    for case in range(80):
        a = _random_stack(rng)
        sk = R.thin(a)
        assert sk.shape == a.shape and sk.dtype == np.uint8
        assert ((sk == a) | (sk == 0)).all(), case                   # a subset of the input
        assert np.array_equal(R.thin(sk), sk), case                  # idempotent
        union = np.zeros_like(a)
        for v in np.unique(a[a != 0]):
            one = R.thin(np.where(a == v, v, 0).astype(np.uint8))
            assert not (union[one != 0]).any()
            union |= one
            for f in range(a.shape[0]):                              # the 8-connected components of every value are kept
                assert R.components_count(a[f] == v) == R.components_count(sk[f] == v), (case, v, f)
        assert np.array_equal(union, sk), case                       # the union of the per-value binary results
        prev = a
        for k in range(1, 5):                                        # nested in max_iterations
            cur = R.thin(a, max_iterations=k)
            assert ((cur == prev) | (cur == 0)).all() and ((sk == cur) | (sk == 0)).all(), (case, k)
            prev = cur


def test_tiled_evaluation_equals_the_global_one():
    rng = np.random.default_rng(7)
    for case in range(12):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 70))
        a = R.blobs(case, 1, H, W)[0] if case % 2 else rng.integers(0, 3, (H, W)).astype(np.uint8)
        for th, tw, k, count, first in ((8, 12, 4, 11, 0), (5, 7, 2, 6, 1), (16, 16, 6, 13, 3)):
            assert np.array_equal(R.thin_tiled(a, th, tw, k, count, first), R.run(a, first, count)[0]), (case, th, tw, k)


def test_longest_path():
    from rmem_ocu_amd import skeleton
    from rmem_ocu_amd._lib import RmemError

    def raster(pts):
        return np.array(sorted(pts), dtype=np.int64)

    cases = [
        # a line: the far end from the first pixel, and back
        (raster([(2, x) for x in range(5)]), [[2, 4], [2, 3], [2, 2], [2, 1], [2, 0]]),
        # a T: (0, 4) and (3, 2) are both 4 hops from (0, 0), the smaller raster index wins; from (0, 4), (0, 0) and (3, 2) tie again
        (raster([(0, x) for x in range(5)] + [(y, 2) for y in range(1, 4)]), [[0, 4], [0, 3], [0, 2], [0, 1], [0, 0]]),
        # a plus: from (4, 2) the search discovers (2, 3) before (2, 2) (NE before N), and (2, 3) discovers (1, 2)
        (raster([(2, x) for x in range(5)] + [(y, 2) for y in (0, 1, 3, 4)]), [[4, 2], [3, 2], [2, 3], [1, 2], [0, 2]]),
        # a loop of six: a long path, not a diameter of a tree
        (raster([(0, 1), (0, 2), (1, 0), (1, 3), (2, 1), (2, 2)]), [[2, 2], [1, 3], [0, 2], [0, 1]]),
        (raster([(3, 4)]), [[3, 4]]),
    ]
    for yx, want in cases:
        for fn in (skeleton.longest_path, R.longest_path):
            got = fn(yx)
            assert got.dtype == np.int32 and got.tolist() == want, (fn, want)
    yx = raster([(0, 0), (0, 1), (5, 5), (5, 6), (5, 7)])
    assert skeleton.component(yx, 3).tolist() == [2, 3, 4] and skeleton.component(yx, 0).tolist() == [0, 1]
    for bad in (np.zeros((0, 2)), np.zeros((3,)), np.zeros((3, 3))):
        with pytest.raises(RmemError, match='yx must be a non-empty'):
            skeleton.longest_path(bad)


def _scribbles(frames):
    return [{v: (d['positive'], d['depth2'], d['path'].tolist()) for v, d in f.items()} for f in frames]


def test_next_scribbles_on_hand_made_stacks():
    z = np.zeros((1, 9, 13), dtype=np.uint8)
    bar = z.copy()
    bar[0, 2:7, 2:11] = 1                                            # 5 x 9: the middle row is 3 deep, its skeleton columns 4..8
    mid = [[4, 8], [4, 7], [4, 6], [4, 5], [4, 4]]
    assert _scribbles(R.next_scribbles(bar, bar, 2)) == [{}]                                     # no error
    assert _scribbles(R.next_scribbles(z, bar, 2)) == [{1: (True, 9, mid)}]                      # false negatives only
    assert _scribbles(R.next_scribbles(bar, z, 2)) == [{1: (False, 9, mid)}]                     # false positives only
    assert _scribbles(R.next_scribbles(z, bar * 3, 2)) == [{}]                                   # a value above num_objs
    gt, pred = np.zeros((1, 13, 13), dtype=np.uint8), np.zeros((1, 13, 13), dtype=np.uint8)
    gt[0, 1:6, 2:11] = 2
    pred[0, 7:12, 2:11] = 2                                          # equal depth: the false positive
    assert _scribbles(R.next_scribbles(pred, gt, 2)) == [{2: (False, 9, [[9, 8], [9, 7], [9, 6], [9, 5], [9, 4]])}]
    gt[0, 0:7, 2:11] = 2                                             # 7 rows from the frame's top edge: 4 deep, the edge counts
    assert _scribbles(R.next_scribbles(pred, gt, 2)) == [{2: (True, 16, [[3, 7], [3, 6], [3, 5]])}]
    sliver = z.copy()
    sliver[0, 4, 2:11] = 1                                           # one pixel wide: depth2 1
    assert _scribbles(R.next_scribbles(z, sliver, 2)) == [{}]
    sliver[0, 3:6, 2:11] = 1                                         # three wide: depth2 4, the default threshold
    assert _scribbles(R.next_scribbles(z, sliver, 2)) == [{1: (True, 4, [[4, x] for x in range(9, 2, -1)])}]
    assert _scribbles(R.next_scribbles(z, sliver, 2, min_depth2=5)) == [{}]
    edge = z.copy()
    edge[0, 0:5, 0:9] = 1                                            # in the frame's corner: the outside is another value
    assert _scribbles(R.next_scribbles(z, edge, 2)) == [{1: (True, 9, [[2, 6], [2, 5], [2, 4], [2, 3], [2, 2]])}]


def test_workspace_sizes(lib):
    th, tw, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.rmem_label_thin_tile(th, tw, k) == 0
    th, tw = th.value, tw.value
    # the second stack in 16-byte units, then two bytes per tile and frame in 16-byte units
    tiles = -(-37 // th) * -(-131 // tw)
    assert lib.rmem_label_thin_workspace_bytes(2, 37, 131) == (2 * 37 * 131 + 15) // 16 * 16 + (2 * 2 * tiles + 15) // 16 * 16
    assert (th, tw, k.value) == (48, 112, 8) and lib.rmem_label_thin_workspace_bytes(2, 37, 131) == 9696 + 16
    assert lib.rmem_label_thin_workspace_bytes(1, 1, 1) == 32
    # 8 bytes per frame, then one counter per unit of 4096 pixels and frame, each in 16-byte units
    assert lib.rmem_label_pixels_workspace_bytes(2, 37, 131) == 16 + 16
    assert lib.rmem_label_pixels_workspace_bytes(3, 150, 200) == 32 + (3 * 8 * 4 + 15) // 16 * 16
    for n, H, W in ((0, 3, 5), (65536, 3, 5), (1, 0, 5), (1, 3, -1), (1, 16384, 16384)):
        assert lib.rmem_label_thin_workspace_bytes(n, H, W) == 0, (n, H, W)
        assert lib.rmem_label_pixels_workspace_bytes(n, H, W) == 0, (n, H, W)


def test_c_entry_points_refuse_on_the_host(lib):
    """non-zero, a message, and nothing launched: the pointers are never looked through"""
    P, n, H, W = 4096, 2, 3, 5                                       # a non-null, aligned address
    need = lib.rmem_label_thin_workspace_bytes(n, H, W)

    def thin(labels=P, n=n, H=H, W=W, first=0, count=2, out=P, lost=P, ws=P, ws_bytes=need):
        return lib.rmem_label_thin(labels, n, H, W, first, count, out, lost, ws, ws_bytes, None)

    for kw, msg in ((dict(labels=None), b'null pointer'), (dict(out=None), b'null pointer'), (dict(lost=None), b'null pointer'),
                    (dict(ws=None), b'null pointer'), (dict(n=0), b'n must be'), (dict(n=65536), b'n must be'),
                    (dict(H=0), b'must be positive'), (dict(W=-1), b'must be positive'), (dict(n=1, H=16384, W=16384), b'at most 2^26'),
                    (dict(first=-1), b'first must not be negative'), (dict(count=0), b'count must be at least 1'),
                    (dict(first=2 ** 31 - 1, count=1), b'must fit 31 bits'), (dict(ws_bytes=need - 1), b'workspace too small'),
                    (dict(ws=P + 2), b'4-byte aligned')):
        assert thin(**kw) != 0, kw
        assert b'rmem_label_thin:' in lib.rmem_last_error_string() and msg in lib.rmem_last_error_string(), (kw, lib.rmem_last_error_string())
    pneed = lib.rmem_label_pixels_workspace_bytes(n, H, W)

    def count(stack=P, n=n, H=H, W=W, totals=P, ws=P, ws_bytes=pneed):
        return lib.rmem_label_pixels_count(stack, n, H, W, totals, ws, ws_bytes, None)

    def write(stack=P, samples=None, n=n, H=H, W=W, capacity=4, entries=P, sampled=None, ws=P, ws_bytes=pneed):
        return lib.rmem_label_pixels_write(stack, samples, n, H, W, capacity, entries, sampled, ws, ws_bytes, None)

    for kw, msg in ((dict(stack=None), b'null pointer'), (dict(totals=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                    (dict(n=0), b'n must be'), (dict(H=0), b'must be positive'), (dict(n=1, H=16384, W=16384), b'at most 2^26'),
                    (dict(ws_bytes=pneed - 1), b'workspace too small'), (dict(ws=P + 4), b'8-byte aligned')):
        assert count(**kw) != 0, kw
        assert b'rmem_label_pixels_count:' in lib.rmem_last_error_string() and msg in lib.rmem_last_error_string(), kw
    for kw, msg in ((dict(stack=None), b'null pointer'), (dict(entries=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                    (dict(samples=P), b'samples and sampled go together'), (dict(sampled=P), b'samples and sampled go together'),
                    (dict(n=65536), b'n must be'), (dict(W=0), b'must be positive'), (dict(capacity=-1), b'capacity must not be negative'),
                    (dict(ws_bytes=pneed - 1), b'workspace too small'), (dict(ws=P + 4), b'8-byte aligned')):
        assert write(**kw) != 0, kw
        assert b'rmem_label_pixels_write:' in lib.rmem_last_error_string() and msg in lib.rmem_last_error_string(), kw
    buf = (ctypes.c_ubyte * 32)()
    assert lib.rmem_label_thin_table(2, buf) != 0 and b'parity must be 0 or 1' in lib.rmem_last_error_string()
    assert lib.rmem_label_thin_table(0, None) != 0 and b'null pointer' in lib.rmem_last_error_string()
    assert lib.rmem_label_thin_tile(None, None, None) != 0 and b'null pointer' in lib.rmem_last_error_string()


def test_python_functions_refuse_on_the_host():
    from rmem_ocu_amd import evaluator, skeleton
    from rmem_ocu_amd._lib import RmemError
    host = torch.zeros(2, 3, 5, dtype=torch.uint8)
    with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
        skeleton.thin(host)
    with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
        skeleton.thin(host.int())
    for bad in (-1, 1.5, True, 2 ** 29 + 1):
        with pytest.raises(RmemError, match='max_iterations must be None or an integer'):
            skeleton.thin(host, max_iterations=bad)
    for bad in (0, 1, 3, 2.0, True, 2 ** 20 + 2):
        with pytest.raises(RmemError, match='batch must be an even integer'):
            skeleton.thin(host, batch=bad)
    with pytest.raises(RmemError, match='stack must be a uint8 device tensor'):
        skeleton.pixels(host)
    for bad in (2, -1, True, 0.0):
        with pytest.raises(RmemError, match='parity must be 0 or 1'):
            skeleton.table(bad)
    for bad in (0, 256, 1.5, True):
        with pytest.raises(RmemError, match='num_objs must be an integer in 1..255'):
            evaluator.next_scribbles(host, host, bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(RmemError, match='min_depth2 must be an integer'):
            evaluator.next_scribbles(host, host, 3, min_depth2=bad)
    with pytest.raises(RmemError, match='must be a uint8 device tensor'):
        evaluator.next_scribbles(host, host, 3)
    with pytest.raises(RmemError, match='must be a uint8 device tensor'):
        evaluator.next_scribbles(host.float(), host.float(), 3)
