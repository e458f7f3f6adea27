"""The shape census on the MI355X against tests/shapes_ref.py: exact equality of the three tables (moments, row extents, hull
vertices and offsets) everywhere.  Shapes: W odd, rows shorter than one 16-byte load and longer than one step of the row loop,
more corner levels than a workgroup has threads and than the hull walk loads at a time, one full-size frame, rows of 16384 equal
pixels and a frame 16384 rows high (the hull walk's LDS at its largest).
Labels sit between guard bytes at byte offsets 0, 1 and 5 and are read only; outputs are pre-filled with 0xA5 and followed by
guard words."""
import functools

import numpy as np
import pytest
import torch

import census_ref
import shapes_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
CANARY64 = int(np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0])
NUM = 10
SHAPES = [(1, 1, 1), (1, 1, 17), (3, 5, 33), (2, 37, 131), (4, 64, 256), (1, 3, 2100), (1, 300, 40), (1, 1100, 6), (1, 480, 854)]
CONTENTS = ['zero', 'all 255', 'random', 'blobs', 'corners', 'stripes', 'discs', 'staircase', 'cee', 'two pieces', 'single', 'borders']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _stack(shape, content):
    """the label stack of one (shape, content): computed once, shared, read only"""
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    a = np.zeros(shape, dtype=np.uint8)
    if content == 'all 255':                                       # a value above NUM: in the moments, in no extent or hull
        a[:] = 255
    elif content == 'random':                                      # 0..11 (11 is above NUM too) with some 255
        a = rng.integers(0, 12, shape).astype(np.uint8)
        a[rng.random(shape) < 0.02] = 255
    elif content == 'blobs':
        a = census_ref.blobs(H * W + n, n, H, W)
    elif content == 'corners':                                     # one value in the four corner pixels only: the hull is the frame
        a[:, 0, 0] = a[:, 0, W - 1] = a[:, H - 1, 0] = a[:, H - 1, W - 1] = 7
    elif content == 'stripes':                                     # vertical stripes one pixel wide: every lane's 16 bytes are mixed
        a[:] = (np.arange(W) % 3 + 1).astype(np.uint8)[None, None, :]
    elif content == 'discs':                                       # many hull vertices; radius 230 at 480 x 854
        r = min(H, W) * 0.48
        for f in range(n):
            a[f][R.disc(H, W, H / 2 - 0.5 + f, W / 2 - 0.5, r)] = 1
            a[f][R.disc(H, W, H * 0.3, W * 0.25 + f, r * 0.45)] = 2
            a[f][R.disc(H, W, H - 1, W - 1, r * 0.3)] = 3          # clipped by two borders
    elif content == 'staircase':                                   # a one-pixel diagonal, and its mirror image
        for y in range(H):
            a[:, y, y * W // H] = 4
            if (W - 1 - y * W // H) != y * W // H:
                a[:, y, W - 1 - y * W // H] = 5
    elif content == 'cee':                                         # concave: a 'C' open to the right
        a[:, H // 8:H - H // 8, W // 8:W - W // 8] = 6
        a[:, H // 3:H - H // 3, W // 3:] = 0
    elif content == 'two pieces':                                  # two far pieces of one value
        a[:, :max(H // 6, 1), :max(W // 5, 1)] = 8
        a[:, H - max(H // 4, 1):, W - max(W // 7, 1):] = 8
    elif content == 'single':                                      # a single pixel, a single row, a single column
        a[:, H // 2, W // 3] = 1
        a[:, H - 1, :] = 2
        a[:, :H - 1, W - 1] = 3
    elif content == 'borders':                                     # an object touching all four borders, and one inside it
        a[:] = 9
        a[:, 1:H - 1, 1:W - 1] = 0
        a[:, H // 4:H // 2, W // 4:W // 2] = 10
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(shape, content):
    a = _stack(shape, content)
    verts, off = R.hulls(a, NUM)
    return R.moments(a), R.extents(a, NUM), verts, off


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _tables(dev, a, num, offset=0, together=True):
    """the entry points on a guarded copy of a, every output pre-filled with 0xA5 and followed by guard words ->
    (moments, extents, verts, offsets) as numpy arrays.  together: moments and extents from one call, else from two"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = a.shape
    s = torch.cuda.current_stream(dev).cuda_stream
    buf, view, front = _guarded(dev, a, offset)
    nm, ne, nf, no = n * 256 * 6, n * num * H * 2, n * num * (H + 1), n * num + 1
    mom = torch.full((nm + 64,), CANARY64, dtype=torch.int64, device=dev)
    ext = torch.full((ne + 64,), CANARY32, dtype=torch.int32, device=dev)
    flags = torch.full((nf + 64,), CANARY, dtype=torch.uint8, device=dev)
    off = torch.full((no + 64,), CANARY32, dtype=torch.int32, device=dev)
    if together:
        _lib.check(L.rmem_label_moments(view.data_ptr(), n, H, W, num, mom.data_ptr(), ext.data_ptr(), s), 'rmem_label_moments')
    else:
        _lib.check(L.rmem_label_moments(view.data_ptr(), n, H, W, 0, mom.data_ptr(), None, s), 'rmem_label_moments')
        _lib.check(L.rmem_label_moments(view.data_ptr(), n, H, W, num, None, ext.data_ptr(), s), 'rmem_label_moments')
    _lib.check(L.rmem_label_hull_count(ext.data_ptr(), n, H, W, num, flags.data_ptr(), off.data_ptr(), s), 'rmem_label_hull_count')
    _lib.check(L.rmem_label_hull_offsets(off.data_ptr(), n * num, s), 'rmem_label_hull_offsets')
    o = off.cpu().numpy()
    V = int(o[no - 1])
    assert 0 <= V <= 2 * (H + 1) * n * num and (o[no:] == CANARY32).all(), 'the total, and ints beyond the offsets'
    verts = torch.full((2 * V + 64,), CANARY32, dtype=torch.int32, device=dev)
    if V:
        _lib.check(L.rmem_label_hull_write(ext.data_ptr(), flags.data_ptr(), n, H, W, num, off.data_ptr(), verts.data_ptr(), V, s), 'rmem_label_hull_write')
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:front] == CANARY).all() and (b[front + a.size:] == CANARY).all(), 'guard bytes around the labels'
    assert np.array_equal(b[front:front + a.size], a.reshape(-1)), 'the labels are read only'
    m, e, fl, v = mom.cpu().numpy(), ext.cpu().numpy(), flags.cpu().numpy(), verts.cpu().numpy()
    assert (m[nm:] == CANARY64).all() and (e[ne:] == CANARY32).all() and (fl[nf:] == CANARY).all() and (v[2 * V:] == CANARY32).all(), 'guard words'
    assert (fl[:nf] <= 3).all()
    return m[:nm].reshape(n, 256, 6), e[:ne].reshape(n, num, H, 2), v[:2 * V].reshape(V, 2), o[:no]


def _assert_tables(got, want, note=''):
    for name, g, w in zip(('moments', 'extents', 'verts', 'offsets'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (note, name, g.shape, w.shape,
                                                                                    np.argwhere(g != w)[:6] if g.shape == w.shape else None)


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_shapes(dev, shape, content):
    a, want = _stack(shape, content), _ref(shape, content)
    for offset in (0, 1, 5):
        _assert_tables(_tables(dev, a, NUM, offset, together=offset != 1), want, offset)


@pytest.mark.parametrize('shape', [(1, 2, 16384), (1, 64, 16384), (1, 16384, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_label_shapes_long_uniform_rows(dev, shape):
    """rows of 16384 equal pixels: 32-bit row or workgroup partial sums would wrap; 16384 rows: the hull walk's LDS at its largest.
    Against closed forms."""
    n, H, W = shape
    a = np.full(shape, 3, dtype=np.uint8)
    mom, ext, verts, off = _tables(dev, a, NUM)
    want = np.zeros((1, 256, 6), dtype=np.int64)
    want[0, 3] = R.uniform_moments(H, W)
    assert max(R.uniform_moments(H, W)) > 2 ** 32 and np.array_equal(mom, want), (mom[0, 3], want[0, 3])
    want_ext = np.empty((1, NUM, H, 2), dtype=np.int32)
    want_ext[..., 0], want_ext[..., 1] = W, -1
    want_ext[0, 2] = (0, W - 1)
    assert np.array_equal(ext, want_ext)
    assert verts.tolist() == [[0, 0], [W, 0], [W, H], [0, H]] and off.tolist() == [0, 0, 0] + [4] * (NUM - 2)


def _wrapped(dev, a, num, **kw):
    from rmem_ocu_amd import shapes
    t = torch.from_numpy(a.copy()).to(dev)
    verts, off = shapes.convex_hulls(t, num, **kw)
    return shapes.label_moments(t).cpu().numpy(), shapes.row_extents(t, num).cpu().numpy(), verts.cpu().numpy(), off.cpu().numpy()


def test_wrappers_reuse_a_dirty_workspace_and_reproduce(dev):
    """the same calls on different stacks one after the other share the (device, stream) workspace; two runs are bit-identical"""
    from rmem_ocu_amd import shapes
    for shape in ((4, 64, 256), (2, 37, 131)):
        for content in ('discs', 'random', 'zero', 'blobs'):
            got = _wrapped(dev, _stack(shape, content), NUM)
            assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32 and got[3].dtype == np.int32
            _assert_tables(got, _ref(shape, content), (shape, content))
    t = torch.from_numpy(_stack((1, 480, 854), 'random').copy()).to(dev)
    runs = [(shapes.label_moments(t), shapes.row_extents(t, NUM)) + shapes.convex_hulls(t, NUM) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert tuple(shapes.label_moments(t[0]).shape) == (1, 256, 6) and tuple(shapes.row_extents(t[0], 3).shape) == (1, 3, 480, 2)


def test_small_workspace_forces_passes(dev):
    from rmem_ocu_amd import shapes
    from rmem_ocu_amd._lib import RmemError
    shape = (4, 64, 256)
    per_frame = shapes.frame_bytes(64, NUM)
    for content in ('discs', 'blobs'):
        want = _ref(shape, content)
        for ws in (per_frame, 3 * per_frame + 5):                  # four passes of one frame; a pass of three and one of one
            _assert_tables(_wrapped(dev, _stack(shape, content), NUM, workspace_bytes=ws), want, (content, ws))
    t = torch.from_numpy(_stack(shape, 'blobs').copy()).to(dev)
    with pytest.raises(RmemError, match='workspace_bytes'):
        shapes.convex_hulls(t, NUM, workspace_bytes=per_frame - 1)
    with pytest.raises(RmemError, match='too large'):
        shapes.label_moments(torch.zeros(1, 1, 16385, dtype=torch.uint8, device=dev))


@functools.lru_cache(maxsize=None)
def _clip():
    a = census_ref.blobs(11, 3, 37, 131, ids=(1, 2, 3, 4, 6)).copy()
    a[1][R.disc(37, 131, 18, 90, 14)] = 5
    a[2, 3, 7] = 7
    a[0][a[0] == 2] = 0                                             # object 2 is absent from frame 0
    a[:, 36, 100:] = 255
    a.setflags(write=False)
    return a


def test_region_props_and_evaluator_wrappers(dev):
    from rmem_ocu_amd import shapes
    from rmem_ocu_amd.evaluator import object_centroids, object_shapes, rotated_boxes
    from test_shapes_host import _assert_props_equal
    a = _clip()
    t = torch.from_numpy(a.copy()).to(dev)
    want = R.stack_props(a, 7)
    _assert_props_equal(shapes.region_props(t, 7), want)
    _assert_props_equal(shapes.region_props(t, 7, workspace_bytes=shapes.frame_bytes(37, 7)), want)
    _assert_props_equal(object_shapes(t, 7), want)
    sq = [0, 40, 41, 42, 43, 44]
    got = object_shapes(t, 7, squeeze_idx=sq)
    _assert_props_equal(got, R.stack_props(a, 7, sq))
    assert sorted(got[1]) == [41, 42, 43, 44] and sorted(got[0]) == [42, 43]        # object 1 lies under the others; 6 and 7 have no key
    c, b = object_centroids(t, 7), rotated_boxes(t, 7)
    assert c.dtype == np.float64 and c.shape == (3, 7, 2) and b.dtype == np.float64 and b.shape == (3, 7, 8)
    for f in range(3):
        for v in range(1, 8):
            if v in want[f]:
                assert tuple(c[f, v - 1]) == want[f][v]['centroid']
                assert np.allclose(b[f, v - 1], want[f][v]['min_rect'].reshape(-1), rtol=1e-12, atol=0.0)
            else:
                assert np.isnan(c[f, v - 1]).all() and np.isnan(b[f, v - 1]).all()
    assert np.isnan(c[0, 1]).all() and not np.isnan(c[2, 6]).any()
