"""Connected components on the MI355X against tests/components_ref.py (scipy.ndimage.label): exact integer equality everywhere and
a status word of 0 in every case.  The stack sits between guard bytes and starts at any byte, the outputs are dirtied first and
followed by guard ints, the shapes aim at the seams of the tile the library reports, the contents at long paths, at pieces of one
pixel and at representatives that have to travel across seams.  Content and references are computed once per case."""
import functools
import warnings

import numpy as np
import pytest
import torch

import census_ref
import components_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
FULL = (1, 480, 854)
CONTENTS = ['zero', 'blobs', 'speckle', 'noise', 'checker', 'hstripes', 'vstripes', 'serpentine', 'rings', 'nest', 'ell']
RULES = [(0, 0, False), (8, 0, False), (0, 8, False), (16, 16, False), (0, 0, True), (-1, -1, True)]      # -1: H * W


@functools.lru_cache(maxsize=None)
def _tile():
    from rmem_ocu_amd import components
    return components.tile()


def _shapes():
    th, tw = _tile()
    return [(1, 1, 1), (1, 1, 17), (2, 3, 5), (1, th, tw), (1, th + 1, tw + 1), (2, 2 * th + 3, 2 * tw + 5), (3, 37, 131)]


SHAPE_IDS = ['1x1x1', '1x1x17', '2x3x5', 'one tile', 'tile+1', 'four seams', '3x37x131']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _content(shape, content):
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    y, x = np.mgrid[0:H, 0:W]
    if content == 'zero':
        a = np.zeros(shape, dtype=np.uint8)
    elif content == 'blobs':
        a = census_ref.blobs(H * W + n, n, H, W)
    elif content == 'speckle':                                      # blobs and 0.2 % of the pixels thrown to any of 0..10, one at least
        a = census_ref.blobs(H * W + n, n, H, W)
        hit = rng.random(shape) < 0.002
        hit[:, H // 2, W // 2] = True
        a[hit] = rng.integers(0, 11, shape).astype(np.uint8)[hit]
    elif content == 'noise':                                        # nearly every pixel is its own piece
        a = rng.integers(0, 4, shape).astype(np.uint8)
    elif content == 'checker':                                      # 4: every pixel a piece; 8: two pieces that span every seam
        a = np.broadcast_to(((y + x) % 2).astype(np.uint8), shape).copy()
    elif content == 'hstripes':
        a = np.broadcast_to((y % 2).astype(np.uint8), shape).copy()
    elif content == 'vstripes':
        a = np.broadcast_to((x % 2).astype(np.uint8), shape).copy()
    elif content == 'serpentine':                                   # one piece of 1 whose inner path is as long as a frame allows
        s = (y % 2 == 0) | ((y % 4 == 1) & (x == W - 1)) | ((y % 4 == 3) & (x == 0))
        a = np.broadcast_to(s.astype(np.uint8), shape).copy()
    elif content == 'rings':
        d = np.maximum(np.abs(y - H // 2), np.abs(x - W // 2))
        a = np.broadcast_to(((d // 2) % 3).astype(np.uint8), shape).copy()
    elif content == 'nest':                                         # 1 holding 0 holding 2 holding one pixel of 0
        a = np.zeros(shape, dtype=np.uint8)
        for k, v in enumerate((1, 0, 2)):
            my, mx = (k + 1) * H // 9 + k, (k + 1) * W // 9 + k
            a[:, my:H - my, mx:W - mx] = v
        a[:, H // 2, W // 2] = 0
    else:                                                           # 'ell': entered from the right -- the first raster pixel lies in the
        a = np.zeros(shape, dtype=np.uint8)                         # last tile column, the piece ends in the first one
        a[:, :, W - 1] = 5
        a[:, H - 1, :] = 5
        a[:, 0, W - 1] = 0 if H > 2 else 5
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(shape, content, conn):
    """(roots, stats, table) of one case: computed once, shared, read only"""
    a = _content(shape, content)
    r = R.roots(a, conn)
    S, T = R.stats(a, conn, r)
    for t in (r, S, T):
        t.setflags(write=False)
    return r, S, T


def _ref_clean(shape, content, conn, rule):
    r, S, T = _ref(shape, content, conn)
    HW = shape[1] * shape[2]
    hole, speck, largest = rule
    return R.clean(_content(shape, content), HW if hole < 0 else hole, HW if speck < 0 else speck, largest, conn, r, (S, T))


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _guards_intact(buf, front, size):
    h = buf.cpu().numpy()
    return (h[:front] == CANARY).all() and (h[front + size:] == CANARY).all()


def _dirty(dev, size):
    return torch.full((size + 64,), CANARY32, dtype=torch.int32, device=dev)


def _run(dev, a, conn, offset=0, want_stats=True):
    """the two entry points on a guarded copy of a -> (roots, stats, table) as numpy; outputs dirtied and guarded, status 0"""
    from rmem_ocu_amd import _lib
    n, H, W = a.shape
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    buf, view, front = _guarded(dev, a, offset)
    roots, status = _dirty(dev, a.size), torch.zeros(1 + 64, dtype=torch.int32, device=dev)
    status[1:] = CANARY32
    _lib.check(L.rmem_label_components(view.data_ptr(), n, H, W, conn, roots.data_ptr(), status.data_ptr(), stream), 'rmem_label_components')
    stats = table = None
    if want_stats:
        stats, table = _dirty(dev, a.size * 4), _dirty(dev, n * 768)
        _lib.check(L.rmem_label_component_stats(view.data_ptr(), roots.data_ptr(), n, H, W, conn, stats.data_ptr(), table.data_ptr(), stream),
                   'rmem_label_component_stats')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, a.size), 'guard bytes around the stack'
    assert np.array_equal(buf[front:front + a.size].cpu().numpy(), a.reshape(-1)), 'the stack is read only'
    st = status.cpu().numpy()
    assert st[0] == 0 and (st[1:] == CANARY32).all(), f'status {st[0]}'
    out = []
    for t, size, shape in ((roots, a.size, a.shape), (stats, a.size * 4, (n, H * W, 4)), (table, n * 768, (n, 256, 3))):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[size:] == CANARY32).all(), 'ints beyond an output were written'
        out.append(h[:size].reshape(shape))
    return out


def _check(dev, shape, content, conn, offset=0, want_stats=True):
    a = _content(shape, content)
    r, S, T = _ref(shape, content, conn)
    got_r, got_S, got_T = _run(dev, a, conn, offset, want_stats)
    assert np.array_equal(got_r, r), (content, conn, offset, np.argwhere(got_r != r)[:8])
    if want_stats:
        assert np.array_equal(got_S, S), (content, conn, offset, np.argwhere(got_S != S)[:8])
        assert np.array_equal(got_T, T), (content, conn, offset, np.argwhere(got_T != T)[:8])


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('k', range(7), ids=SHAPE_IDS)
def test_components_and_stats(dev, k, content):
    """roots, stats and table as whole arrays, both connectivities, the stack starting at every byte offset"""
    shape = _shapes()[k]
    for conn in (4, 8):
        for offset in OFFSETS:
            _check(dev, shape, content, conn, offset)


def test_contents_are_what_they_claim():
    """the checkerboard's and the serpentine's piece counts, and the L's first pixel, by the reference"""
    th, tw = _tile()
    shape = (2, 2 * th + 3, 2 * tw + 5)
    n, H, W = shape
    assert _ref(shape, 'checker', 4)[2][0, :2, 0].tolist() == [(H * W + 1) // 2, H * W // 2]
    assert _ref(shape, 'checker', 8)[2][0, :2, 0].tolist() == [1, 1]
    for conn in (4, 8):
        assert _ref(shape, 'serpentine', conn)[2][0, 1].tolist() == [1, int(_content(shape, 'serpentine')[0].sum()), 0]
        r, _, T = _ref(shape, 'ell', conn)
        assert T[0, 5].tolist() == [1, H + W - 2, 2 * W - 1] and r[0, H - 1, 0] == 2 * W - 1 and (2 * W - 1) % W >= tw


@pytest.mark.parametrize('content', ['blobs', 'noise'])
def test_full_size_frame(dev, content):
    for conn in (4, 8):
        _check(dev, FULL, content, conn, 13)
        for offset in (0, 1, 3):
            _check(dev, FULL, content, conn, offset, want_stats=False)


def _clean(dev, a, rule, conn, **kw):
    from rmem_ocu_amd.components import clean_labels
    HW = a.shape[1] * a.shape[2]
    hole, speck, largest = rule
    return clean_labels(a, HW if hole < 0 else hole, HW if speck < 0 else speck, largest, conn, **kw)


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('k', range(7), ids=SHAPE_IDS)
def test_clean_labels_rules(dev, k, content):
    """every rule against the reference; in place equals out of place"""
    shape = _shapes()[k]
    a = _content(shape, content)
    d = torch.from_numpy(a.copy()).to(dev)
    for conn in (4, 8):
        for rule in RULES:
            want = _ref_clean(shape, content, conn, rule)
            got = _clean(dev, d, rule, conn)
            assert got.dtype == torch.uint8 and got.shape == d.shape and got.data_ptr() != d.data_ptr()
            assert np.array_equal(got.cpu().numpy(), want), (content, conn, rule, np.argwhere(got.cpu().numpy() != want)[:8])
            assert np.array_equal(d.cpu().numpy(), a), 'the input is read only'
            if rule == RULES[0]:
                assert np.array_equal(want, a), 'the identity'
            inplace = d.clone()
            back = _clean(dev, inplace, rule, conn, out=inplace)
            assert back is inplace and np.array_equal(inplace.cpu().numpy(), want), (content, conn, rule, 'in place')


@pytest.mark.parametrize('content', ['blobs', 'noise'])
def test_clean_labels_full_size_frame(dev, content):
    a = _content(FULL, content)
    d = torch.from_numpy(a.copy()).to(dev)
    for conn in (4, 8):
        for rule in RULES:
            got = _clean(dev, d, rule, conn).cpu().numpy()
            want = _ref_clean(FULL, content, conn, rule)
            assert np.array_equal(got, want), (content, conn, rule, np.argwhere(got != want)[:8])


def test_clean_entry_point_at_byte_offsets(dev):
    """rmem_label_clean itself: src and dst between guard bytes at every pair of offsets, dst dirtied, out of place and in place"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    th, tw = _tile()
    for shape in ((2, 3, 5), (2, 2 * th + 3, 2 * tw + 5)):
        n, H, W = shape
        a = _content(shape, 'speckle')
        r, S, T = (torch.from_numpy(t.copy()).to(dev) for t in _ref(shape, 'speckle', 8))
        want = _ref_clean(shape, 'speckle', 8, (16, 16, True))
        assert not np.array_equal(want, a)
        for so in OFFSETS:
            for do in OFFSETS:
                sbuf, sview, sfront = _guarded(dev, a, so)
                dbuf, dview, dfront = _guarded(dev, np.full(shape, CANARY, dtype=np.uint8), do)
                _lib.check(L.rmem_label_clean(sview.data_ptr(), dview.data_ptr(), r.data_ptr(), S.data_ptr(), T.data_ptr(), n, H, W, 16, 16, 1,
                                              stream), 'rmem_label_clean')
                torch.cuda.synchronize()
                assert _guards_intact(sbuf, sfront, a.size) and _guards_intact(dbuf, dfront, a.size), (so, do)
                assert np.array_equal(sview.cpu().numpy(), a) and np.array_equal(dview.cpu().numpy(), want), (so, do)
            _lib.check(L.rmem_label_clean(sview.data_ptr(), sview.data_ptr(), r.data_ptr(), S.data_ptr(), T.data_ptr(), n, H, W, 16, 16, 1,
                                          stream), 'rmem_label_clean')
            torch.cuda.synchronize()
            assert _guards_intact(sbuf, sfront, a.size) and np.array_equal(sview.cpu().numpy(), want), (so, 'in place')


def test_python_functions(dev):
    """label_components, component_stats and object_fragments through the package, [H, W] as one frame"""
    from rmem_ocu_amd import components
    from rmem_ocu_amd.evaluator import clean_masks, object_fragments
    shape = (3, 37, 131)
    for content in ('speckle', 'noise'):
        d = torch.from_numpy(_content(shape, content).copy()).to(dev)
        for conn in (4, 8):
            r, S, T = _ref(shape, content, conn)
            roots, status = components.label_components(d, conn)
            assert roots.dtype == torch.int32 and roots.shape == d.shape and status.dtype == torch.int32 and status.shape == (1,)
            stats, table = components.component_stats(d, roots, conn)
            assert stats.shape == (3, 37 * 131, 4) and table.shape == (3, 256, 3) and int(status.item()) == 0
            assert np.array_equal(roots.cpu().numpy(), r) and np.array_equal(stats.cpu().numpy(), S) and np.array_equal(table.cpu().numpy(), T)
            for frag in (components.object_fragments(d, 10, conn), object_fragments(d, 10, conn)):
                assert frag.dtype == torch.int32 and frag.shape == (3, 11) and np.array_equal(frag.cpu().numpy(), T[:, :11, 0])
            one, _ = components.label_components(d[1], conn)
            assert one.shape == (1, 37, 131) and np.array_equal(one.cpu().numpy()[0], r[1])
        got = clean_masks(d, fill_holes=16, remove_specks=16, keep_largest=True)
        assert np.array_equal(got.cpu().numpy(), _ref_clean(shape, content, 8, (16, 16, True)))
        assert np.array_equal(clean_masks(d[2], 8, 0).cpu().numpy(), _ref_clean(shape, content, 8, (8, 0, False))[2])
    x = torch.zeros(2, 4, 4, dtype=torch.uint8, device=dev)
    from rmem_ocu_amd._lib import RmemError
    with pytest.raises(RmemError, match='out must be a tensor of the labels\' shape'):
        components.clean_labels(x, out=x[:1])
    with pytest.raises(RmemError, match='out must be a contiguous uint8 tensor'):
        components.clean_labels(x, out=x.int())
    with pytest.raises(RmemError, match='status must be an int32 tensor'):
        components.clean_labels(x, status=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RmemError, match='workspace_bytes'):
        components.clean_labels(x, workspace_bytes=16)
    with pytest.raises(RmemError, match='roots must be'):
        components.component_stats(x, x)


def test_workspace_passes_and_reuse(dev):
    """one frame per pass equals the default; calls of different shapes share one workspace and equal fresh results"""
    from rmem_ocu_amd import _lib
    th, tw = _tile()
    big, small = (2, 2 * th + 3, 2 * tw + 5), (3, 37, 131)
    rule = (16, 16, True)
    per_frame = int(_lib.lib().rmem_label_components_workspace_bytes(1, big[1], big[2]))
    d_big = torch.from_numpy(_content(big, 'speckle').copy()).to(dev)
    d_small = torch.from_numpy(_content(small, 'noise').copy()).to(dev)
    w_big, w_small = _ref_clean(big, 'speckle', 8, rule), _ref_clean(small, 'noise', 8, rule)
    assert np.array_equal(_clean(dev, d_big, rule, 8).cpu().numpy(), w_big)
    assert np.array_equal(_clean(dev, d_big, rule, 8, workspace_bytes=per_frame).cpu().numpy(), w_big)
    assert np.array_equal(_clean(dev, d_big, rule, 8, workspace_bytes=2 * per_frame - 1).cpu().numpy(), w_big)
    for _ in range(2):                                              # small after big after small: a dirty, larger workspace never shows
        assert np.array_equal(_clean(dev, d_small, rule, 8).cpu().numpy(), w_small)
        assert np.array_equal(_clean(dev, d_big, rule, 8).cpu().numpy(), w_big)
    per_small = int(_lib.lib().rmem_label_components_workspace_bytes(1, small[1], small[2]))
    assert np.array_equal(_clean(dev, d_small, rule, 8, workspace_bytes=2 * per_small).cpu().numpy(), w_small)      # passes of 2 + 1 frames


def test_clean_labels_with_a_status_tensor_makes_no_host_sync(dev, monkeypatch):
    """with the caller's status word nothing in clean_labels waits for the device: every synchronising call raises meanwhile"""
    from rmem_ocu_amd.components import clean_labels
    shape = (3, 37, 131)
    d = torch.from_numpy(_content(shape, 'speckle').copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty_like(d)
    clean_labels(d, 16, 16, True, out=out)                          # the workspace exists now
    torch.cuda.synchronize()
    out.fill_(CANARY)

    def refuse(*a, **k):
        raise AssertionError('a host synchronisation inside clean_labels')

    with monkeypatch.context() as m:
        for owner, name in ((torch.Tensor, 'item'), (torch.Tensor, 'cpu'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'),
                            (torch.Tensor, '__bool__'), (torch.Tensor, '__int__'), (torch.cuda, 'synchronize'),
                            (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
            m.setattr(owner, name, refuse)
        with pytest.raises(AssertionError, match='host synchronisation'):       # the check bites: status=None reads the word back
            clean_labels(d, 16, 16, True, out=out)
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                         # "a prototype feature": it may miss a sync, the patches above do not
            torch.cuda.set_sync_debug_mode('error')
        try:
            got = clean_labels(d, 16, 16, True, out=out, workspace_bytes=None, status=status)
        finally:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert got is out and int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy(), _ref_clean(shape, 'speckle', 8, (16, 16, True)))
