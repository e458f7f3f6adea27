"""The thinning of label stacks, the pixel list and the scribbles on the MI355X against tests/skeleton_ref.py: exact equality of
whole arrays everywhere.  The stack sits between guard bytes and starts at any byte, outputs and workspace are dirtied first and
followed by guard bytes.  The shapes are the smallest that can go wrong: one pixel, one row, one column, frames of several tiles in
either direction, seams placed from skeleton.tile().  Content and references are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import skeleton_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 3, 5), (3, 17, 33), (2, 37, 131), (1, 40, 1100), (1, 1100, 40), (1, 150, 200)]
CONTENTS = ['one', 'blobs', 'noise', 'dots', 'full', 'hstripes2', 'hstripes3', 'vstripes2', 'vstripes3', 'last', 'border', 'void', 'absent']
DIRECT = ['blobs', 'noise', 'full', 'border']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _tile():
    from rmem_ocu_amd import skeleton
    return skeleton.tile()


@functools.lru_cache(maxsize=None)
def _content(shape, content):
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    y, x = np.mgrid[0:H, 0:W]
    a = np.zeros(shape, dtype=np.uint8)
    if content == 'one':                                             # one value in one blob
        a[:, H // 4:H - H // 4, W // 4:W - W // 4] = 3
    elif content == 'blobs':
        a = R.blobs(H * W + n, n, H, W)
    elif content == 'noise':
        a = rng.integers(0, 4, shape).astype(np.uint8)
    elif content == 'dots':                                          # one-pixel objects
        hit = (y % 4 == 1) & (x % 5 == 2)
        a[:, hit] = (1 + (y + x) % 3).astype(np.uint8)[hit]
        a[:, H // 2, W // 2] = 3
    elif content == 'full':                                          # a full frame
        a[:] = 1
    elif content in ('hstripes2', 'hstripes3', 'vstripes2', 'vstripes3'):
        w = int(content[-1])
        c = y if content[0] == 'h' else x
        a[:] = np.where(c // w % 2 == 0, 1 + c // w % 3, 0).astype(np.uint8)
    elif content == 'last':                                          # objects on the last row, the last column and the corner
        a[:, H - 2:, :(W + 1) // 2] = 1
        a[:, :(H + 1) // 2, W - 2:] = 2
        a[:, H - 1, W - 1] = 3
    elif content == 'border':                                        # two values sharing a long border
        a[:] = np.where(x + y // 3 < (W + H // 3) // 2, 1, 2).astype(np.uint8)
    elif content == 'void':                                          # value 255 next to another
        a = np.where(R.blobs(H + W, n, H, W, values=2) == 1, 255, 0).astype(np.uint8)
        a[:, :, W // 2:][a[:, :, W // 2:] == 0] = 7
    elif content == 'absent':                                        # even frames empty
        a = R.blobs(H * W + 3 * n, n, H, W)
        a[0::2] = 0
    elif content == 'zero':
        pass
    else:
        raise KeyError(content)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _skeleton(shape, content):
    sk = R.thin(_content(shape, content))
    sk.setflags(write=False)
    return sk


def _guarded(dev, a, offset, fill=None):
    """a's bytes (or `fill` bytes in their place) on the device between guard bytes, starting `offset` bytes past a 64-byte
    boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    if fill is None:
        buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _guards_intact(buf, front, size):
    h = buf.cpu().numpy()
    return (h[:front] == CANARY).all() and (h[front + size:] == CANARY).all()


def _call_thin(dev, src, dst, first, count, ws=None, stream=None):
    """rmem_label_thin on device views; the workspace dirtied and followed by guard bytes -> lost [n, 2] as numpy"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = src.shape
    need = int(L.rmem_label_thin_workspace_bytes(n, H, W))
    assert need >= src.numel()
    if ws is None:
        ws = torch.full((need + 64,), CANARY, dtype=torch.uint8, device=dev)
    lost = torch.full((2 * n + 16,), CANARY32, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
    _lib.check(L.rmem_label_thin(src.data_ptr(), n, H, W, first, count, dst.data_ptr(), lost.data_ptr(), ws.data_ptr(), need, st),
               'rmem_label_thin')
    torch.cuda.synchronize()
    assert bool((ws[need:] == CANARY).all().item()), 'bytes beyond the workspace were written'
    assert bool((lost[2 * n:] == CANARY32).all().item()), 'ints beyond lost were written'
    return lost[:2 * n].cpu().numpy().reshape(n, 2)


def _direct(dev, a, first, count, offset=0):
    """a guarded copy of a thinned into a dirtied, guarded output -> (out, lost)"""
    buf, view, front = _guarded(dev, a, offset)
    obuf, out, ofront = _guarded(dev, a, (offset * 5 + 2) % 16, fill=CANARY)
    lost = _call_thin(dev, view, out, first, count)
    assert _guards_intact(buf, front, a.size) and _guards_intact(obuf, ofront, a.size), 'guard bytes around the stacks'
    assert np.array_equal(buf[front:front + a.size].cpu().numpy(), a.reshape(-1)), 'the stack is read only'
    return out.cpu().numpy(), lost


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_thin_equals_the_reference(dev, shape, content):
    from rmem_ocu_amd import skeleton
    a = _content(shape, content)
    t = torch.from_numpy(a.copy()).to(dev)
    got = skeleton.thin(t)
    assert got.shape == t.shape and got.dtype == torch.uint8 and got.data_ptr() != t.data_ptr()
    assert np.array_equal(got.cpu().numpy(), _skeleton(shape, content))
    assert np.array_equal(t.cpu().numpy(), a), 'the input is left alone'


@pytest.mark.parametrize('content', DIRECT)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_direct_calls_between_guards(dev, shape, content):
    """the C entry point: any byte offset, dirtied output and workspace, lost against the reference's counts; an odd count across a
    round boundary and a single sub-iteration of odd parity"""
    k = _tile()[2]
    a = _content(shape, content)
    offset = OFFSETS[(SHAPES.index(shape) + DIRECT.index(content)) % 4]
    for first, count in ((0, k + 3), (1, 1)):
        want, want_lost = R.run(a, first, count)
        got, lost = _direct(dev, a, first, count, offset)
        assert np.array_equal(got, want), (first, count)
        assert np.array_equal(lost, want_lost), (first, count)


@pytest.mark.parametrize('offset', OFFSETS)
def test_every_byte_offset(dev, offset):
    a = _content((2, 37, 131), 'blobs')
    k = _tile()[2]
    got, lost = _direct(dev, a, 0, 2 * k, offset)
    want, want_lost = R.run(a, 0, 2 * k)
    assert np.array_equal(got, want) and np.array_equal(lost, want_lost)


@functools.lru_cache(maxsize=None)
def _seams(case):
    th, tw, k = _tile()
    if case == 'disk':                                               # a disk on a four-tile corner, radius above k: several rounds
        r = k + 5
        H, W = th + r + 3, tw + r + 3
        y, x = np.mgrid[0:H, 0:W]
        a = (((y - th) ** 2 + (x - tw) ** 2 <= r * r) * 5).astype(np.uint8)[None]
    elif case == 'bar':                                              # a bar that crosses three tiles
        a = np.zeros((1, 2 * k + 7, 2 * tw + 9), dtype=np.uint8)
        a[0, 3:2 * k + 4, 2:2 * tw + 7] = 2
    elif case == 'tall':                                             # the same downward
        a = np.zeros((1, 2 * th + 9, 2 * k + 7), dtype=np.uint8)
        a[0, 2:2 * th + 7, 3:2 * k + 4] = 2
    elif case == 'plus1':                                            # a width one more than a multiple of the tile
        a = R.blobs(11, 1, th + 1, 2 * tw + 1, count=9)
    elif case == 'minus1':
        a = R.blobs(12, 1, th - 1, 2 * tw - 1, count=9)
    else:
        raise KeyError(case)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize('case', ['disk', 'bar', 'tall', 'plus1', 'minus1'])
def test_seams_from_the_tile(dev, case):
    from rmem_ocu_amd import skeleton
    a = _seams(case)
    k = _tile()[2]
    want, iterations = R.thin(a, with_iterations=True)
    if case == 'disk':
        assert iterations == k + 6 and 2 * iterations > k             # radius r: r + 1 iterations, more than one round
    assert np.array_equal(skeleton.thin(torch.from_numpy(a.copy()).to(dev)).cpu().numpy(), want)
    got, lost = _direct(dev, a, 0, 3 * k + 1, 3)
    want, want_lost = R.run(a, 0, 3 * k + 1)
    assert np.array_equal(got, want) and np.array_equal(lost, want_lost)


@pytest.mark.parametrize('case', ['disk', 'blobs'])
def test_max_iterations(dev, case):
    from rmem_ocu_amd import skeleton
    k = _tile()[2]
    a = _seams('disk') if case == 'disk' else _content((2, 37, 131), 'blobs')
    t = torch.from_numpy(a.copy()).to(dev)
    for it in sorted({1, 2, k // 2 - 1, k // 2, k // 2 + 1, k + 1}):   # the short last round and the round boundary
        assert np.array_equal(skeleton.thin(t, max_iterations=it).cpu().numpy(), R.thin(a, max_iterations=it)), it
    assert np.array_equal(skeleton.thin(t, max_iterations=0).cpu().numpy(), a)
    out = torch.full_like(t, CANARY)
    assert skeleton.thin(t, max_iterations=3, out=out) is out and np.array_equal(out.cpu().numpy(), R.thin(a, max_iterations=3))


@pytest.mark.parametrize('case', ['disk', 'blobs'])
def test_chained_calls_in_place(dev, case):
    """odd first, odd count, in place with odd and even numbers of rounds: the chain equals one long call, every call's lost the
    reference's"""
    k = _tile()[2]
    a = _seams('disk') if case == 'disk' else _content((2, 37, 131), 'blobs')
    buf, view, front = _guarded(dev, a, 5)
    state, first = a, 0
    for count in (3, 5, 1, 2 * k + 1, k + 2, 2 * k, 2):
        lost = _call_thin(dev, view, view, first, count)
        state, want_lost = R.run(state, first, count)
        assert np.array_equal(view.cpu().numpy(), state), (first, count)
        assert np.array_equal(lost, want_lost), (first, count)
        first += count
    assert _guards_intact(buf, front, a.size)
    assert np.array_equal(state, R.run(a, 0, first)[0])
    assert np.array_equal(_direct(dev, a, 0, first)[0], state)


def test_batches_converge_to_one_stack(dev):
    from rmem_ocu_amd import skeleton
    k = _tile()[2]
    for a in (_seams('disk'), _content((3, 17, 33), 'blobs'), _content((1, 40, 1100), 'full')):
        t = torch.from_numpy(a.copy()).to(dev)
        want = R.thin(a)
        for batch in (2, k, 64):
            assert np.array_equal(skeleton.thin(t, batch=batch).cpu().numpy(), want), batch
        work = t.clone()
        assert skeleton.thin(work, out=work) is work and np.array_equal(work.cpu().numpy(), want)      # in place


def test_side_stream_twice(dev):
    a = _content((2, 37, 131), 'noise')
    k = _tile()[2]
    want, want_lost = R.run(a, 0, 2 * k + 1)
    side = torch.cuda.Stream(dev)
    t = torch.from_numpy(a.copy()).to(dev)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        out = torch.full_like(t, CANARY)
        torch.cuda.synchronize()
        lost = _call_thin(dev, t, out, 0, 2 * k + 1, stream=side)
        outs.append((out.cpu().numpy(), lost))
    for got, lost in outs:
        assert np.array_equal(got, want) and np.array_equal(lost, want_lost)


def test_one_frame_per_pass(dev):
    from rmem_ocu_amd import _lib, skeleton
    a = _content((3, 17, 33), 'blobs')
    t = torch.from_numpy(a.copy()).to(dev)
    one = int(_lib.lib().rmem_label_thin_workspace_bytes(1, 17, 33))
    want = _skeleton((3, 17, 33), 'blobs')
    assert np.array_equal(skeleton.thin(t, workspace_bytes=one).cpu().numpy(), want)
    assert np.array_equal(skeleton.thin(t, max_iterations=2, workspace_bytes=one).cpu().numpy(), R.thin(a, max_iterations=2))
    with pytest.raises(_lib.RmemError, match='workspace_bytes must be an integer of at least'):
        skeleton.thin(t, workspace_bytes=one - 1)


def test_idle_tile_switch(dev, monkeypatch):
    """the experiment switch: with and without the idle-tile skip the stacks and the counters are the same"""
    k = _tile()[2]
    for a in (_seams('disk'), _seams('bar'), _content((1, 150, 200), 'blobs'), _content((1, 40, 1100), 'dots')):
        want, want_lost = R.run(a, 0, 6 * k + 1)
        for value in ('0', '1', None):
            if value is None:
                monkeypatch.delenv('RMEM_THIN_SKIP', raising=False)
            else:
                monkeypatch.setenv('RMEM_THIN_SKIP', value)
            got, lost = _direct(dev, a, 0, 6 * k + 1)
            assert np.array_equal(got, want) and np.array_equal(lost, want_lost), value
            buf, view, front = _guarded(dev, a, 1)                   # in place: the first round reads the buffer the second writes
            lost = _call_thin(dev, view, view, 0, 6 * k)
            assert np.array_equal(view.cpu().numpy(), R.run(a, 0, 6 * k)[0]) and np.array_equal(lost, R.run(a, 0, 6 * k)[1]), value


@pytest.mark.parametrize('content', CONTENTS + ['zero'])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 5), (3, 17, 33), (2, 37, 131), (1, 150, 200)], ids=lambda s: 'x'.join(map(str, s)))
def test_pixels(dev, shape, content):
    from rmem_ocu_amd import _lib, skeleton
    a = _content(shape, content)
    n, H, W = shape
    samples = (np.arange(a.size, dtype=np.int64).reshape(shape) * 7 % 1000003).astype(np.int32)
    want_e, want_t, want_s = R.pixels(a, samples)
    buf, view, front = _guarded(dev, a, OFFSETS[(H + W) % 4])
    ts = torch.from_numpy(samples).to(dev)
    e, t = skeleton.pixels(view)
    assert e.dtype == torch.int32 and t.dtype == torch.int32 and tuple(e.shape) == (len(want_e), 4)
    assert np.array_equal(e.cpu().numpy(), want_e) and np.array_equal(t.cpu().numpy(), want_t)
    e, t, s = skeleton.pixels(view, samples=ts)
    assert np.array_equal(e.cpu().numpy(), want_e) and np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(s.cpu().numpy(), want_s)
    assert _guards_intact(buf, front, a.size)
    # a capacity below the total: totals stay exact, nothing is written beyond the capacity
    L = _lib.lib()
    total, cap = len(want_e), len(want_e) // 2
    need = int(L.rmem_label_pixels_workspace_bytes(n, H, W))
    ws = torch.full((need + 64,), CANARY, dtype=torch.uint8, device=dev)
    totals = torch.full((n + 16,), CANARY32, dtype=torch.int32, device=dev)
    entries = torch.full((total + 16, 4), CANARY32, dtype=torch.int32, device=dev)
    sampled = torch.full((total + 16,), CANARY32, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.rmem_label_pixels_count(view.data_ptr(), n, H, W, totals.data_ptr(), ws.data_ptr(), need, st), 'rmem_label_pixels_count')
    _lib.check(L.rmem_label_pixels_write(view.data_ptr(), ts.data_ptr(), n, H, W, cap, entries.data_ptr(), sampled.data_ptr(), ws.data_ptr(),
                                         need, st), 'rmem_label_pixels_write')
    torch.cuda.synchronize()
    assert np.array_equal(totals[:n].cpu().numpy(), want_t) and bool((totals[n:] == CANARY32).all().item())
    assert np.array_equal(entries[:cap].cpu().numpy(), want_e[:cap]) and bool((entries[cap:] == CANARY32).all().item())
    assert np.array_equal(sampled[:cap].cpu().numpy(), want_s[:cap]) and bool((sampled[cap:] == CANARY32).all().item())
    assert bool((ws[need:] == CANARY).all().item())


def test_pixels_refuses_bad_samples(dev):
    from rmem_ocu_amd import skeleton
    from rmem_ocu_amd._lib import RmemError
    t = torch.zeros(2, 3, 5, dtype=torch.uint8, device=dev)
    for bad in (torch.zeros(2, 3, 5, device=dev), torch.zeros(2, 3, 4, dtype=torch.int32, device=dev), torch.zeros(2, 3, 5, dtype=torch.int32)):
        with pytest.raises(RmemError, match='samples must be an int32 tensor of the stack\'s shape'):
            skeleton.pixels(t, samples=bad)
    with pytest.raises(RmemError, match='out must be a contiguous uint8 tensor'):
        skeleton.thin(t, out=torch.zeros(2, 3, 4, dtype=torch.uint8, device=dev))


def _same_scribbles(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for v in w:
            assert g[v]['positive'] is w[v]['positive'] or g[v]['positive'] == w[v]['positive']
            assert g[v]['depth2'] == w[v]['depth2'] and isinstance(g[v]['depth2'], int)
            assert g[v]['path'].dtype == np.int32 and np.array_equal(g[v]['path'], w[v]['path'])


def _hand_made():
    z = np.zeros((1, 9, 13), dtype=np.uint8)
    bar = z.copy()
    bar[0, 2:7, 2:11] = 1
    gt, pred = np.zeros((1, 13, 13), dtype=np.uint8), np.zeros((1, 13, 13), dtype=np.uint8)
    gt[0, 1:6, 2:11] = 2
    pred[0, 7:12, 2:11] = 2
    deep = gt.copy()
    deep[0, 0:7, 2:11] = 2
    sliver, three, edge = z.copy(), z.copy(), z.copy()
    sliver[0, 4, 2:11] = 1
    three[0, 3:6, 2:11] = 1
    edge[0, 0:5, 0:9] = 1
    return [(bar, bar, 2, 4), (z, bar, 2, 4), (bar, z, 2, 4), (z, bar * 3, 2, 4), (pred, gt, 2, 4), (pred, deep, 2, 4), (z, sliver, 2, 4),
            (z, three, 2, 4), (z, three, 2, 5), (z, edge, 2, 4), (z[0], edge[0], 1, 0)]


def test_next_scribbles(dev):
    from rmem_ocu_amd import evaluator
    for pred, gt, num, depth in _hand_made():
        got = evaluator.next_scribbles(torch.from_numpy(pred.copy()).to(dev), torch.from_numpy(gt.copy()).to(dev), num, min_depth2=depth)
        _same_scribbles(got, R.next_scribbles(pred, gt, num, depth))
    gt = R.blobs(77, 2, 37, 131, values=10, count=16)                # 10 objects, the prediction moved by (3, 5)
    pred = np.roll(gt, (3, 5), axis=(1, 2))
    want = R.next_scribbles(pred, gt, 10)
    assert sum(len(f) for f in want) >= 4
    _same_scribbles(evaluator.next_scribbles(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), 10), want)
    _same_scribbles(evaluator.next_scribbles(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), 10, min_depth2=1),
                    R.next_scribbles(pred, gt, 10, 1))
