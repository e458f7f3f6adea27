"""The ring simplifier on the MI355X against tests/polysimplify_ref.py (the sequential restatement of the contract): rings_s[:R],
verts_s[:V_out] and counts_s as whole arrays, exact equality, no tolerance anywhere.  Outputs and workspace are dirtied first and
followed by guards; the tables are traced contents, hand-made rings on the seam between the two kernels (one wave per ring, one
workgroup per ring), rings whose recursion is as deep as they are long, keys next to 2^62 and damaged tables.  References are
computed once per case and shared."""
import functools
import warnings

import numpy as np
import pytest
import torch

import components_ref
import polygons_ref as P
import polysimplify_ref as S

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
K = 10
SHAPES = [(1, 1, 1), (1, 1, 17), (2, 3, 5), (2, 67, 133), (3, 37, 131)]
TOLERANCES = (0, 0.5, 1, 2.5, 64)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _content(name, shape, num_objs=K):
    a = S.content(name, shape, num_objs)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _traced(name, shape, conn, num_objs=K):
    out = P.arrays(_content(name, shape, num_objs), num_objs, conn)
    for t in out:
        t.setflags(write=False)
    return out


def _dirty(dev, size):
    return torch.full((size + 64,), CANARY32, dtype=torch.int32, device=dev)


def _run(dev, table, T, MR=None, MV=None, ws=None):
    """the entry point on a table (rings, verts, counts as numpy) in tensors of MR and MV rows -> (rings_s [MR, 8], verts_s
    [MV, 2], counts_s [4]) as numpy, pre-fill included; outputs and workspace are dirtied first and every guard is looked at"""
    from rmem_ocu_amd import _lib
    rings, verts, counts = (np.array(t, dtype=np.int32) for t in table)
    MR = max(1, len(rings)) if MR is None else MR
    MV = max(1, len(verts)) if MV is None else MV
    L = _lib.lib()
    need = int(L.rmem_polygon_simplify_workspace_bytes(MR, MV))
    assert need > 0
    if ws is None:
        ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=dev)
    assert ws.numel() >= need + 256
    tail = ws[need:].clone()
    r_in, v_in = np.full((MR, 8), CANARY32, dtype=np.int32), np.full((MV, 2), CANARY32, dtype=np.int32)
    r_in[:min(MR, len(rings))], v_in[:min(MV, len(verts))] = rings[:MR], verts[:MV]
    d = [torch.from_numpy(t).to(dev) for t in (r_in, v_in, counts)]
    outs = [_dirty(dev, MR * 8), _dirty(dev, MV * 2), _dirty(dev, 4)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.rmem_polygon_simplify(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), MR, MV, int(T), ws.data_ptr(), need,
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), stream), 'rmem_polygon_simplify')
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], tail), 'bytes beyond the workspace were written'
    for t, h in zip(d, (r_in, v_in, counts)):
        assert np.array_equal(t.cpu().numpy(), h), 'the input is read only'
    got = []
    for t, size in zip(outs, (MR * 8, MV * 2, 4)):
        g = t.cpu().numpy()
        assert (g[size:] == CANARY32).all(), 'ints beyond an output were written'
        got.append(g[:size])
    return got[0].reshape(MR, 8), got[1].reshape(MV, 2), got[2]


def _same(got, want, what):
    rings, verts, counts = got
    w_rings, w_verts, w_counts = want
    assert counts.tolist() == w_counts.tolist(), (what, counts.tolist(), w_counts.tolist())
    R_, V_ = int(w_counts[1]), int(w_counts[2])
    assert np.array_equal(rings[:R_], w_rings), (what, np.argwhere(rings[:R_] != w_rings)[:8])
    assert np.array_equal(verts[:V_], w_verts), (what, np.argwhere(verts[:V_] != w_verts)[:8])
    assert (rings[R_:] == CANARY32).all() and (verts[V_:] == CANARY32).all(), (what, 'rows beyond R or V_out were written')


def _check(dev, table, T, what, **kw):
    MR, MV = kw.get('MR'), kw.get('MV')
    want = S.simplify_arrays(*table, T, max_rings=MR if MR is not None else max(1, len(table[0])),
                             max_verts=MV if MV is not None else max(1, len(table[1])))
    got = _run(dev, table, T, **kw)
    _same(got, want, what)
    return got


# ------------------------------------------------------------------------------------------------------------- traced contents
@pytest.mark.parametrize('name', S.CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_whole_arrays(dev, shape, name):
    """every content, both connectivities, every tolerance: the three arrays equal the restatement's"""
    for conn in (4, 8):
        table = _traced(name, shape, conn)
        R, V = len(table[0]), len(table[1])
        for k, tol in enumerate(TOLERANCES):
            extra = {} if k % 2 == 0 else {'MR': R + 3, 'MV': V + 5}            # the exact fit and a little room
            _check(dev, table, S.steps(tol), (name, shape, conn, tol), **extra)


def test_full_size_frame(dev):
    """one 480 x 854 blob frame at one pixel: most vertices go, the long outlines take the workgroup kernel"""
    from rmem_ocu_amd import polygons
    table = _traced('blobs', (1, 480, 854), 8, 3)
    assert int(table[0][:, 3].max()) > polygons.short_max()
    got = _check(dev, table, 16, 'full size')
    assert 0 < got[2][2] < table[2][2] // 4


# -------------------------------------------------------------------------------------------------------------- hand-made tables
BIG = [(0, 0), (16383, 1), (32767, 0), (32765, 16383), (32767, 32767), (16383, 32766), (0, 32767), (2, 16383)]


def test_teeth_on_the_seam_and_deep(dev):
    """refinement as deep as the ring is long, in both kernels and on either side of the seam between them"""
    from rmem_ocu_amd import polygons
    short = polygons.short_max()
    assert short % 2 == 0 and short >= 8
    at_seam, beyond = S.teeth((short - 4) // 2, pad=1), S.teeth((short - 2) // 2)
    assert len(at_seam) == short and len(beyond) == short + 1
    for ring in (at_seam, beyond, S.teeth(400), S.teeth((short - 4) // 2), S.teeth(130, pad=7)):
        for T in (0, 8, 16, 40, 200, 1024):
            _check(dev, S.table([ring]), T, (len(ring), T))
    # both classes in one table
    for T in (8, 24):
        _check(dev, S.table([at_seam, beyond, at_seam]), T, ('pair', T))


def test_tiny_and_equal_rings(dev):
    rings = [[(7, 9)], [(7, 9), (7, 9)], [(0, 0), (3, 0)], [(0, 0), (4, 0), (4, 3)], [(3, 3)] * 5, [(3, 3)] * 70, [(0, 0)] * 64,
             [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)], [(1, 1), (4, 1), (1, 4)], [(0, 0), (10, 0), (7, 2), (3, 2)]]
    for T in (0, 7, 11, 16, 24, 38, 39, 1024):
        _check(dev, S.table(rings), T, ('tiny', T))


def test_keys_next_to_two_to_the_62(dev):
    """corners and edge midpoints of the 32767 square, the midpoints bumped by 1 and 2 pixels: 64-bit products at their largest"""
    far = [(0, 0), (32767, 32767), (0, 32767), (32767, 0), (1, 32766), (32766, 1)]
    assert max(S.key_thr(far[0], far[1], p, 1024)[0] for p in far) > 2 ** 59
    for T in (0, 8, 15, 16, 17, 31, 32, 33, 1024):
        _check(dev, S.table([BIG, far, BIG[::-1], BIG * 9]), T, ('big', T))


def test_rings_alternating_between_the_classes(dev):
    rng = np.random.default_rng(3)
    rings = []
    for k in range(40):
        n = int(rng.integers(1, 40)) if k % 2 == 0 else int(rng.integers(65, 700))
        walk = np.cumsum(rng.integers(-3, 4, size=(n, 2)), axis=0)
        rings.append(walk - walk.min(axis=0))
    rings += [S.teeth(40), SQUARE, S.teeth(31), S.teeth(100, pad=3), SQUARE]
    for T in (0, 8, 16, 40, 160):
        _check(dev, S.table(rings), T, ('alternating', T))


SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]


# ---------------------------------------------------------------------------------------------------------------- damaged tables
def _base_table():
    return S.table([S.teeth(20), SQUARE, S.teeth(50), BIG, S.teeth(10)])


def test_damaged_vertices_and_rows(dev):
    """the status bits, the bad ring with 0 vertices, the others still right (the restatement says what 'right' is)"""
    from rmem_ocu_amd import polygons
    clean = _check(dev, _base_table(), 16, 'clean')
    assert clean[2][3] == 0
    for ring, value in ((0, 32768), (2, -1), (1, 40000), (2, 32768)):
        rings, verts, counts = _base_table()
        verts[rings[ring, 2] + 3, ring % 2] = value
        got = _check(dev, (rings, verts, counts), 16, ('vertex', ring, value))
        assert got[2][3] == polygons.SIMPLIFY_ST_RING and got[0][ring, 3] == 0 and got[0][ring, 7] == rings[ring, 3]
        others = [r for r in range(5) if r != ring]
        assert np.array_equal(got[0][others, 3], clean[0][others, 3])
    V = int(_base_table()[2][2])
    for ring, first, count in ((1, None, 0), (1, None, -4), (4, None, 24), (3, -1, None), (2, V, 1), (0, 2 ** 31 - 1, 2 ** 31 - 1)):
        rings, verts, counts = _base_table()
        if first is not None:
            rings[ring, 2] = first
        if count is not None:
            rings[ring, 3] = count
        got = _check(dev, (rings, verts, counts), 16, ('row', ring, first, count))
        assert got[2][3] == polygons.SIMPLIFY_ST_RING and got[0][ring, 3] == 0
        others = [r for r in range(5) if r != ring]
        assert np.array_equal(got[0][others, 3], clean[0][others, 3])


def test_damaged_counts(dev):
    """R above max_rings, V above max_verts, an input status: the status, R = V_out = 0 and untouched outputs"""
    from rmem_ocu_amd import polygons
    rings, verts, counts = _base_table()
    R, V = len(rings), len(verts)
    for c, want in (([V, R + 1, V, 0], [V, 0, 0, polygons.SIMPLIFY_ST_TABLE]), ([V, R, V + 1, 0], [V + 1, 0, 0, polygons.SIMPLIFY_ST_TABLE]),
                    ([V, -1, V, 0], [V, 0, 0, polygons.SIMPLIFY_ST_TABLE]), ([V, R, -2, 0], [-2, 0, 0, polygons.SIMPLIFY_ST_TABLE]),
                    ([12345, 0, 0, polygons.ST_CAPACITY], [0, 0, 0, polygons.ST_CAPACITY]), ([V, R, V, polygons.ST_LINK], [V, 0, 0, polygons.ST_LINK])):
        got = _check(dev, (rings, verts, np.array(c, dtype=np.int32)), 16, c)
        assert got[2].tolist() == want and (got[0] == CANARY32).all() and (got[1] == CANARY32).all()
    # rings that share vertices: they are simplified while their counts fit max_verts together, refused when they do not
    shared = rings.copy()
    shared[1, 2:4] = (0, 20)
    _check(dev, (shared, verts, counts), 16, 'shared', MV=V + 40)
    got = _check(dev, (shared, verts, counts), 16, 'shared, no room')
    assert got[2].tolist() == [V, 0, 0, polygons.SIMPLIFY_ST_TABLE]


# ----------------------------------------------------------------------------------------------------------------------- hygiene
def test_dirty_workspace_and_identical_bytes(dev):
    from rmem_ocu_amd import _lib
    big, small = _traced('noise', (3, 37, 131), 8), _traced('speckle', (2, 67, 133), 4)
    L = _lib.lib()
    need = max(int(L.rmem_polygon_simplify_workspace_bytes(len(t[0]) + 9, len(t[1]) + 9)) for t in (big, small))
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=dev)
    first = {}
    for rnd in range(2):
        for name, table, T in (('big', big, 16), ('small', small, 8), ('teeth', S.table([S.teeth(300), S.teeth(20)]), 8), ('big', big, 16)):
            got = _check(dev, table, T, (name, rnd), ws=ws)
            key = (name, T)
            if key in first:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(first[key], got))
            first[key] = got


def _device_table(dev, table, MR=None, MV=None):
    rings, verts, counts = table
    r = torch.zeros(max(1, len(rings)) if MR is None else MR, 8, dtype=torch.int32)
    v = torch.zeros(max(1, len(verts)) if MV is None else MV, 2, dtype=torch.int32)
    r[:len(rings)], v[:len(verts)] = torch.from_numpy(np.array(rings)), torch.from_numpy(np.array(verts))
    return r.to(dev), v.to(dev), torch.from_numpy(np.array(counts)).to(dev)


def test_simplify_makes_no_host_sync(dev, monkeypatch):
    """nothing in polygons.simplify waits for the device: every synchronising call raises meanwhile; trace_label_stack, which
    reads counts back, is the control that the patches bite"""
    from rmem_ocu_amd import polygons
    shape = (3, 37, 131)
    labels = torch.from_numpy(_content('speckle', shape).copy()).to(dev)
    table = _traced('speckle', shape, 8)
    want = S.simplify_arrays(*table, 16)
    d = _device_table(dev, table)
    polygons.simplify(*d, 1.0)                                      # the workspace exists now
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('a host synchronisation inside polygons')

    with monkeypatch.context() as m:
        for owner, name in ((torch.Tensor, 'item'), (torch.Tensor, 'cpu'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'),
                            (torch.Tensor, '__bool__'), (torch.Tensor, '__int__'), (torch.cuda, 'synchronize'),
                            (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
            m.setattr(owner, name, refuse)
        with pytest.raises(AssertionError, match='host synchronisation'):
            polygons.trace_label_stack(labels, K, tolerance=1.0)
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            torch.cuda.set_sync_debug_mode('error')
        try:
            rings_s, verts_s, counts_s = polygons.simplify(*d, 1.0)
        finally:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    c = counts_s.cpu().numpy()
    assert c.tolist() == want[2].tolist() and rings_s.shape == d[0].shape and verts_s.shape == d[1].shape
    assert np.array_equal(rings_s[:c[1]].cpu().numpy(), want[0]) and np.array_equal(verts_s[:c[2]].cpu().numpy(), want[1])


def test_simplify_behind_trace_and_device_refusals(dev):
    """polygons.simplify on what polygons.trace left on the device, and the refusals that need a device tensor"""
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    shape = (2, 67, 133)
    for name, conn, tol in (('blobs', 8, 1.5), ('noise', 4, 0.5), ('zero', 8, 1)):
        labels = torch.from_numpy(_content(name, shape).copy()).to(dev)
        table = _traced(name, shape, conn)
        t = polygons.trace(labels, K, conn, max_edges=int(table[2][0]) + 64)    # noise does not fit the default estimate
        rings_s, verts_s, counts_s = polygons.simplify(*t, tol)
        want = S.simplify_arrays(*table, S.steps(tol))
        c = counts_s.cpu().numpy()
        assert c.tolist() == want[2].tolist()
        assert np.array_equal(rings_s[:c[1]].cpu().numpy(), want[0]) and np.array_equal(verts_s[:c[2]].cpu().numpy(), want[1])
    with pytest.raises(RmemError, match='on one device'):
        polygons.simplify(t[0], t[1].cpu(), t[2], 1.0)
    with pytest.raises(RmemError, match='rings must be a contiguous'):
        polygons.simplify(t[0][::2], t[1], t[2], 1.0)


# ------------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('tolerance', [0.5, 1.0, 2.5])
def test_far_pixels_keep_their_value_on_the_device(dev, tolerance):
    """trace -> simplify -> fill_label_stack against the original stack: not one far pixel changes, and a fifth of them are far"""
    from rmem_ocu_amd import polygons
    shape, objs = (2, 67, 133), 3
    a = _content('blobs', shape, objs)
    far = S.far_pixels(a, objs, tolerance)
    assert far.mean() >= 0.2
    for conn in (4, 8):
        frames = polygons.trace_label_stack(torch.from_numpy(a.copy()).to(dev), objs, conn, tolerance=tolerance)
        back = polygons.fill_label_stack([[(v, polys) for v, polys in fr.items() if polys] for fr in frames], shape[1:], dev).cpu().numpy()
        assert np.array_equal(back[far], a[far]), (conn, int((back != a)[far].sum()))
        assert sum(len(p['exterior']) for fr in frames for polys in fr.values() for p in polys) < int(_traced('blobs', shape, conn, objs)[2][2])


def _plain(frames):
    def poly(p):
        return {'exterior': p['exterior'].tolist(), 'area2': p['area2'], 'holes': [h.tolist() for h in p['holes']]}
    return [{k: [poly(p) for p in v] for k, v in fr.items()} for fr in frames]


def _alive(ring):
    ring = [tuple(p) for p in ring]
    return len(ring) >= 3 and sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1])) != 0


def _expected(a, conn, T, degenerate, squeeze_idx=None):
    """the restatement plus group_rings, and the degenerate rule restated on plain lists"""
    from rmem_ocu_amd import polygons
    rings, verts, counts = P.arrays(a, K, conn)
    rs, vs, _ = S.simplify_arrays(rings, verts, counts, T)
    roots = components_ref.roots(a, conn)
    at = np.array([roots[r[0]].reshape(-1)[r[5] >> 2] for r in rs], dtype=np.int32)
    frames = _plain(polygons.group_rings(rs, vs, len(a), K, squeeze_idx, roots_at_start=at))
    if degenerate == 'drop':
        frames = [{k: [dict(p, holes=[h for h in p['holes'] if _alive(h)]) for p in v if _alive(p['exterior'])] for k, v in fr.items()}
                  for fr in frames]
    return frames


def test_trace_label_stack_with_a_tolerance(dev):
    from rmem_ocu_amd import polygons
    shape = (3, 37, 131)
    n, H, W = shape
    for name, conn, tol in (('speckle', 8, 1.0), ('noise', 4, 0.5), ('concentric', 8, 2.5), ('blobs', 4, 1.5)):
        a = _content(name, shape)
        d = torch.from_numpy(a.copy()).to(dev)
        T = S.steps(tol)
        want = _expected(a, conn, T, 'drop')
        keep = _expected(a, conn, T, 'keep')
        assert _plain(polygons.trace_label_stack(d, K, conn, tolerance=tol)) == want
        assert _plain(polygons.trace_label_stack(d, K, conn, tolerance=tol, degenerate='drop')) == want
        assert _plain(polygons.trace_label_stack(d, K, conn, tolerance=tol, degenerate='keep')) == keep
        assert _plain(polygons.trace_label_stack(d, K, conn, max_edges=8, tolerance=tol)) == want              # the retry path
        per = polygons.frame_bytes(H, W, simplified=True)
        assert _plain(polygons.trace_label_stack(d, K, conn, workspace_bytes=per, tolerance=tol)) == want      # one frame per pass
        idx = [0, 40, 7, 9]
        assert _plain(polygons.trace_label_stack(d, K, conn, squeeze_idx=idx, tolerance=tol, degenerate='keep')) == \
            _expected(a, conn, T, 'keep', idx)
        plain = _plain(polygons.trace_label_stack(d, K, conn))
        assert _plain(polygons.trace_label_stack(d, K, conn, tolerance=None)) == plain
        assert _plain(polygons.trace_label_stack(d, K, conn, tolerance=None, degenerate='keep')) == plain
        if name == 'speckle':
            assert keep != want                                     # single pixels do collapse at these tolerances
    assert sum(len(p['exterior']) for fr in want for v in fr.values() for p in v) < sum(len(p['exterior']) for fr in plain for v in fr.values() for p in v)


def test_polygon_results_with_a_tolerance(dev):
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd.evaluator import polygon_results
    shape = (3, 37, 131)
    for name, conn, tol in (('speckle', 8, 1.0), ('concentric', 4, 2.5), ('blobs', 8, 1.5)):
        a = _content(name, shape)
        d = torch.from_numpy(a.copy()).to(dev)
        want = _expected(a, conn, S.steps(tol), 'drop')

        def area2(ring):
            return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]))

        for mode in ('rings', 'drop'):
            got = polygon_results(d, K, None, mode, conn, tolerance=tol)
            assert len(got) == shape[0]
            for f, entry in enumerate(got):
                assert list(entry) == list(range(1, K + 1))
                for k, e in entry.items():
                    polys = want[f][k]
                    assert e['size'] == list(shape[1:]) and e['segmentation'] == [sum(p['exterior'], []) for p in polys]
                    holes = [h for p in polys for h in p['holes']]
                    twice = sum(area2([tuple(v) for v in p['exterior']]) for p in polys)
                    if mode == 'rings':
                        assert e['holes'] == [sum(h, []) for h in holes]
                        twice += sum(area2([tuple(v) for v in h]) for h in holes)
                    else:
                        assert 'holes' not in e
                    assert e['area'] == twice / 2.0 and isinstance(e['area'], float)
        assert polygon_results(d, K, None, 'rings', conn, tolerance=None) == polygon_results(d, K, None, 'rings', conn)
