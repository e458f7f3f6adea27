"""The polygon tracer on the MI355X against tests/polygons_ref.py (the sequential restatement of the contract): rings[:R],
verts[:V] and counts as whole arrays, exact equality.  The stack sits between guard bytes and starts at any byte, the outputs and
the workspace are dirtied first and followed by guards, the shapes aim at the seams of the walk unit the library reports and at
more than one block of every kernel, the contents at saddles, holes inside holes, rings of four edges and one ring that holds
most of a frame's edges.  On every content the device's rings are also checked against the masks themselves (rasterised), the
connected components (outer rings = pieces) and the label census (area).  Content and references are computed once per case."""
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy import ndimage

import census_ref
import polygons_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
FULL = (1, 480, 854)
K = 10                                                              # objects 1..10; the contents hold fewer, or values above
CONTENTS = ['zero', 'full', 'blobs', 'speckle', 'noise', 'checker', 'hstripes', 'vstripes', 'serpentine', 'concentric', 'nest', 'others']


@functools.lru_cache(maxsize=None)
def _unit():
    from rmem_ocu_amd import polygons
    return polygons.unit()


def _shapes():
    u = _unit()
    return [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 3, 5), (1, 1, u), (1, 1, u + 1), (1, 2, u), (2, 67, 133), (3, 37, 131)]


SHAPE_IDS = ['1x1x1', '1x1x17', '1x17x1', '2x3x5', 'one unit', 'unit+1 across', 'unit+1 down', '2x67x133', '3x37x131']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _content(shape, content):
    n, H, W = shape
    seed = n * 7919 + H * 131 + W
    if content == 'zero':
        a = np.zeros(shape, dtype=np.uint8)
    elif content == 'full':
        a = np.full(shape, 3, dtype=np.uint8)
    elif content == 'blobs':
        a = census_ref.blobs(seed, n, H, W)
    elif content == 'speckle':
        a = R.speckle(census_ref.blobs(seed, n, H, W), seed, 0.01, K)
    elif content == 'noise':                                        # saddles everywhere, under both connectivities
        a = R.noise(seed, n, H, W, 4)
    elif content == 'checker':
        a = R.checkerboard(n, H, W)
    elif content == 'hstripes':
        a = R.stripes(2 * n, H, W)[0::2]
    elif content == 'vstripes':
        a = R.stripes(2 * n, H, W)[1::2]
    elif content == 'serpentine':
        a = R.serpentine(n, H, W)
    elif content == 'concentric':
        a = R.concentric(n, H, W)
    elif content == 'nest':
        a = R.nest(n, H, W)
    else:                                                           # 'others': values above num_objs among the objects
        a = R.with_other_values(census_ref.blobs(seed, n, H, W), K, seed)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.shape == shape
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(shape, content, conn):
    """(rings, verts, counts) of one case: computed once, shared, read only"""
    out = R.arrays(_content(shape, content), K, conn)
    for t in out:
        t.setflags(write=False)
    return out


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _dirty(dev, size):
    return torch.full((size + 64,), CANARY32, dtype=torch.int32, device=dev)


def _run(dev, a, conn, M, offset=0):
    """the entry point on a guarded copy of a -> (rings [M // 4 + 1, 8], verts [M, 2], counts [4]) as numpy, pre-fill included;
    the workspace is dirtied too and every guard is looked at"""
    from rmem_ocu_amd import _lib
    n, H, W = a.shape
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    buf, view, front = _guarded(dev, a, offset)
    need = int(L.rmem_label_polygons_workspace_bytes(n, H, W, M))
    assert need > 0
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=dev)
    nr, nv = (M // 4 + 1) * 8, M * 2
    rings, verts, counts = _dirty(dev, nr), _dirty(dev, nv), _dirty(dev, 4)
    _lib.check(L.rmem_label_polygons(view.data_ptr(), n, H, W, K, conn, M, ws.data_ptr(), need, rings.data_ptr(), verts.data_ptr(),
                                     counts.data_ptr(), stream), 'rmem_label_polygons')
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:front] == CANARY).all() and (h[front + a.size:] == CANARY).all(), 'guard bytes around the stack'
    assert np.array_equal(h[front:front + a.size], a.reshape(-1)), 'the stack is read only'
    assert (ws[need:].cpu().numpy() == CANARY).all(), 'bytes beyond the workspace were written'
    out = []
    for t, size in ((rings, nr), (verts, nv), (counts, 4)):
        g = t.cpu().numpy()
        assert (g[size:] == CANARY32).all(), 'ints beyond an output were written'
        out.append(g[:size])
    return out[0].reshape(-1, 8), out[1].reshape(-1, 2), out[2]


def _same(got, want, what):
    rings, verts, counts = got
    w_rings, w_verts, w_counts = want
    assert counts.tolist() == w_counts.tolist(), (what, counts.tolist(), w_counts.tolist())
    R_, V_ = int(w_counts[1]), int(w_counts[2])
    assert np.array_equal(rings[:R_], w_rings), (what, np.argwhere(rings[:R_] != w_rings)[:8])
    assert np.array_equal(verts[:V_], w_verts), (what, np.argwhere(verts[:V_] != w_verts)[:8])
    assert (rings[R_:] == CANARY32).all() and (verts[V_:] == CANARY32).all(), (what, 'rows beyond R or V were written')


def _capacities(shape, E):
    """max_edges per byte offset: the exact fit, the bound, a little above E (the fewest doubling rounds the contract allows)"""
    n, H, W = shape
    return {0: max(4, E), 1: 4 * n * H * W, 3: max(4, E + 7), 13: max(4, E + 1)}


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('k', range(9), ids=SHAPE_IDS)
def test_rings_vertices_and_counts(dev, k, content):
    """whole arrays against the restatement, both connectivities, the stack starting at every byte offset"""
    shape = _shapes()[k]
    a = _content(shape, content)
    for conn in (4, 8):
        want = _ref(shape, content, conn)
        caps = _capacities(shape, int(want[2][0]))
        for offset in OFFSETS:
            _same(_run(dev, a, conn, caps[offset], offset), want, (content, conn, offset))


def _independent(dev, a, conn, rings, verts, counts):
    """the device's rings against the masks, the connected components and the census -- none of them the restatement"""
    from rmem_ocu_amd import components
    from rmem_ocu_amd.protocol import label_census
    n, H, W = a.shape
    d = torch.from_numpy(a.copy()).to(dev)
    roots, _ = components.label_components(d, conn)
    _, table = components.component_stats(d, roots, conn)
    table = table.cpu().numpy()
    area = label_census(d)[0].cpu().numpy()
    rings = rings[:counts[1]]
    for f in range(n):
        mine = R.rings_of(rings, verts, f)
        for v in range(1, K + 1):
            assert np.array_equal(R.rasterise(mine, v, H, W), a[f] == v), (f, v, 'rasterised rings')
            assert sum(r['area2'] > 0 for r in mine if r['value'] == v) == table[f, v, 0], (f, v, 'outer rings = pieces')
            assert sum(r['area2'] for r in mine if r['value'] == v) == 2 * int(area[f, v]), (f, v, 'area')
        assert all(1 <= r['value'] <= K for r in mine)


@pytest.mark.parametrize('content', CONTENTS)
def test_independent_checks(dev, content):
    for shape in ((2, 67, 133), (3, 37, 131), (2, 3, 5)):
        a = _content(shape, content)
        for conn in (4, 8):
            E = int(_ref(shape, content, conn)[2][0])
            _independent(dev, a, conn, *_run(dev, a, conn, max(4, E)))


@pytest.mark.parametrize('conn', [4, 8])
def test_full_size_frame(dev, conn):
    """one 480 x 854 frame of blobs with 10 objects (no noise at this size: the restatement is sequential)"""
    a = _content(FULL, 'blobs')
    want = _ref(FULL, 'blobs', conn)
    got = _run(dev, a, conn, int(want[2][0]) + 7, 13)
    _same(got, want, ('full size', conn))
    _independent(dev, a, conn, *got)


@pytest.mark.parametrize('content', ['speckle', 'checker', 'serpentine', 'full'])
def test_capacity(dev, content):
    """max_edges = E - 1: the status, the exact E, R = V = 0 and untouched outputs; max_edges = E succeeds"""
    from rmem_ocu_amd import polygons
    for shape in ((2, 67, 133), (2, 3, 5)):
        a = _content(shape, content)
        for conn in (4, 8):
            want = _ref(shape, content, conn)
            E = int(want[2][0])
            assert E > 4
            rings, verts, counts = _run(dev, a, conn, E - 1, 1)
            assert counts.tolist() == [E, 0, 0, polygons.ST_CAPACITY]
            assert (rings == CANARY32).all() and (verts == CANARY32).all()
            rings, verts, counts = _run(dev, a, conn, 4, 3)
            assert counts.tolist() == [E, 0, 0, polygons.ST_CAPACITY] and (rings == CANARY32).all() and (verts == CANARY32).all()
            _same(_run(dev, a, conn, E), want, (content, conn, 'exact fit'))


def test_two_calls_give_identical_bytes(dev):
    shape = (3, 37, 131)
    for content in ('noise', 'speckle'):
        a = _content(shape, content)
        M = int(_ref(shape, content, 8)[2][0]) + 100
        first, second = _run(dev, a, 8, M), _run(dev, a, 8, M)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second))


def _trace(dev, shape, content, conn, **kw):
    from rmem_ocu_amd import polygons
    d = torch.from_numpy(_content(shape, content).copy()).to(dev)
    rings, verts, counts = polygons.trace(d, K, conn, **kw)
    return rings.cpu().numpy(), verts.cpu().numpy(), counts.cpu().numpy()


def test_trace_and_shapes_alternating_on_one_workspace(dev):
    """polygons.trace: the tensors' shapes, [H, W] as one frame, and a dirty, larger workspace never shows"""
    from rmem_ocu_amd import polygons
    big, small = (2, 67, 133), (3, 37, 131)
    for _ in range(2):
        for shape, content, conn in ((small, 'speckle', 8), (big, 'noise', 4), (small, 'nest', 4), (big, 'concentric', 8)):
            want = _ref(shape, content, conn)
            M = int(want[2][0]) + 64
            rings, verts, counts = _trace(dev, shape, content, conn, max_edges=M)
            assert rings.shape == (M // 4 + 1, 8) and verts.shape == (M, 2) and counts.shape == (4,)
            assert counts.tolist() == want[2].tolist()
            assert np.array_equal(rings[:counts[1]], want[0]) and np.array_equal(verts[:counts[2]], want[1])
    want = _ref(small, 'blobs', 8)                                   # the default capacity holds blobs
    rings, verts, counts = _trace(dev, small, 'blobs', 8)
    assert verts.shape == (polygons.default_max_edges(*small), 2) and counts.tolist() == want[2].tolist()
    assert np.array_equal(rings[:counts[1]], want[0]) and np.array_equal(verts[:counts[2]], want[1])
    d = torch.from_numpy(_content(small, 'blobs').copy()).to(dev)
    rings, verts, counts = polygons.trace(d[1], K)
    one = R.arrays(_content(small, 'blobs')[1:2], K, 8)
    assert counts.cpu().tolist() == one[2].tolist() and np.array_equal(rings[:one[2][1]].cpu().numpy(), one[0])
    rings, verts, counts = _trace(dev, small, 'checker', 8)        # ... and not a checkerboard: the status says so
    assert counts.tolist() == [int(_ref(small, 'checker', 8)[2][0]), 0, 0, polygons.ST_CAPACITY]
    from rmem_ocu_amd._lib import RmemError
    for bad in (3, 0, 2.5, True, 2 ** 31):
        with pytest.raises(RmemError, match='max_edges must be an integer'):
            polygons.trace(d, K, 8, bad)


def _plain(frames):
    """trace_label_stack's output with lists for arrays"""
    def poly(p):
        return {'exterior': p['exterior'].tolist(), 'area2': p['area2'], 'holes': [h.tolist() for h in p['holes']]}
    return [{k: ([poly(p) for p in v] if k is not None else {'holes': {o: [h.tolist() for h in hs] for o, hs in v['holes'].items()}})
             for k, v in fr.items()} for fr in frames]


def test_trace_label_stack(dev):
    """the host-side product: pieces and their holes against scipy's labelling, a deliberately small max_edges, one frame per
    pass, squeezed keys, and the holes without parents"""
    from rmem_ocu_amd import polygons
    shape = (3, 37, 131)
    n, H, W = shape
    for content, conn in (('speckle', 8), ('noise', 4), ('concentric', 8), ('nest', 4)):
        a = _content(shape, content)
        d = torch.from_numpy(a.copy()).to(dev)
        frames = polygons.trace_label_stack(d, K, conn)
        assert len(frames) == n and all(list(fr) == list(range(1, K + 1)) for fr in frames)
        structure = np.ones((3, 3)) if conn == 8 else ndimage.generate_binary_structure(2, 1)
        for f, fr in enumerate(frames):
            for v in range(1, K + 1):
                pieces, count = ndimage.label(a[f] == v, structure=structure)
                assert len(fr[v]) == count
                for p in fr[v]:                                     # a polygon with its holes is exactly one piece
                    own = [{'value': v, 'verts': r} for r in [p['exterior']] + p['holes']]
                    got = R.rasterise(own, v, H, W)
                    assert p['area2'] == 2 * int(got.sum()) and len(np.unique(pieces[got])) == 1
                    assert int((pieces == pieces[got][0]).sum()) == int(got.sum())
        want = _plain(frames)
        assert _plain(polygons.trace_label_stack(d, K, conn, max_edges=8)) == want
        assert _plain(polygons.trace_label_stack(d, K, conn, workspace_bytes=polygons.frame_bytes(H, W))) == want
        assert _plain(polygons.trace_label_stack(d, K, conn, workspace_bytes=2 * polygons.frame_bytes(H, W))) == want
        idx = [0, 40, 7, 9]
        squeezed = _plain(polygons.trace_label_stack(d, K, conn, squeeze_idx=idx))
        assert squeezed == [{idx[i]: fr[i] for i in (1, 2, 3)} for fr in want]
        loose = polygons.trace_label_stack(d, K, conn, parents=False)
        ref = R.arrays(a, K, conn)
        for f, fr in enumerate(loose):
            mine = R.rings_of(ref[0], ref[1], f)
            for v in range(1, K + 1):
                assert [p['exterior'].tolist() for p in fr[v]] == [r['verts'].tolist() for r in mine if r['value'] == v and r['area2'] > 0]
                assert [h.tolist() for h in fr[None]['holes'][v]] == [r['verts'].tolist() for r in mine if r['value'] == v and r['area2'] < 0]
                assert all(p['holes'] == [] for p in fr[v])
    from rmem_ocu_amd._lib import RmemError
    with pytest.raises(RmemError, match='workspace_bytes'):
        polygons.trace_label_stack(d, K, 8, workspace_bytes=16)


def test_polygon_results(dev):
    """evaluator.polygon_results against the restatement: holes='rings' and 'drop', with and without squeeze_idx"""
    from rmem_ocu_amd.evaluator import polygon_results
    shape = (3, 37, 131)
    n, H, W = shape
    for content, conn in (('speckle', 8), ('concentric', 4)):
        a = _content(shape, content)
        d = torch.from_numpy(a.copy()).to(dev)
        ref = R.arrays(a, K, conn)
        for idx in (None, [0, 40, 7, 9]):
            ids = range(1, K + 1) if idx is None else (1, 2, 3)
            full, drop = polygon_results(d, K, idx, 'rings', conn), polygon_results(d, K, idx, 'drop', conn)
            assert len(full) == len(drop) == n
            for f in range(n):
                mine = R.rings_of(ref[0], ref[1], f)
                assert list(full[f]) == list(drop[f]) == [i if idx is None else idx[i] for i in ids]
                for i in ids:
                    key = i if idx is None else idx[i]
                    outer = [r for r in mine if r['value'] == i and r['area2'] > 0]
                    inner = [r for r in mine if r['value'] == i and r['area2'] < 0]
                    e = full[f][key]
                    assert e['size'] == [H, W] and e['segmentation'] == [r['verts'].reshape(-1).tolist() for r in outer]
                    assert sorted(e['holes']) == sorted(r['verts'].reshape(-1).tolist() for r in inner)
                    assert e['area'] == int((a[f] == i).sum()) == sum(r['area2'] for r in outer + inner) // 2
                    e = drop[f][key]
                    assert e == {'size': [H, W], 'segmentation': [r['verts'].reshape(-1).tolist() for r in outer],
                                 'area': sum(r['area2'] for r in outer) // 2}
    one = polygon_results(d[0], K, connectivity=4)
    assert len(one) == 1 and one[0] == polygon_results(d, K, connectivity=4)[0]


def test_trace_makes_no_host_sync(dev, monkeypatch):
    """nothing in polygons.trace waits for the device: every synchronising call raises meanwhile; trace_label_stack, which reads
    counts back, is the control that the patches bite"""
    from rmem_ocu_amd import polygons
    shape = (3, 37, 131)
    d = torch.from_numpy(_content(shape, 'speckle').copy()).to(dev)
    want = _ref(shape, 'speckle', 8)
    polygons.trace(d, K)                                            # the workspace exists now
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('a host synchronisation inside polygons')

    with monkeypatch.context() as m:
        for owner, name in ((torch.Tensor, 'item'), (torch.Tensor, 'cpu'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'),
                            (torch.Tensor, '__bool__'), (torch.Tensor, '__int__'), (torch.cuda, 'synchronize'),
                            (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
            m.setattr(owner, name, refuse)
        with pytest.raises(AssertionError, match='host synchronisation'):
            polygons.trace_label_stack(d, K)
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                         # "a prototype feature": it may miss a sync, the patches above do not
            torch.cuda.set_sync_debug_mode('error')
        try:
            rings, verts, counts = polygons.trace(d, K)
        finally:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert c.tolist() == want[2].tolist()
    assert np.array_equal(rings[:c[1]].cpu().numpy(), want[0]) and np.array_equal(verts[:c[2]].cpu().numpy(), want[1])
