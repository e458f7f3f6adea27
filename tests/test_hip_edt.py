"""The distance transform of label stacks on the MI355X against tests/edt_ref.py: exact integer equality everywhere, no tolerance.
The stack sits between guard bytes and starts at any byte, outputs and workspace are dirtied first and followed by guard ints.  The
shapes are the smallest that can go wrong: one pixel, one row, one column, rows longer than a workgroup's stride and columns taller
than any band, rows that end on, one before and one after the end of a 32-pixel segment of the row pass (EDGES, also run by
test_hip_nearest and test_hip_surface), and the two 16384-long lines with a single site at index 0 (the largest distances, a
full row image in LDS, a scan as long as the row).  Content and references are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import census_ref
import edt_ref as R

pytestmark = pytest.mark.gpu

S = R.SENTINEL
CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 3, 5), (3, 17, 33), (2, 37, 131), (1, 40, 1100), (1, 1100, 40), (1, 150, 200)]
EDGES = [(2, 3, W) for W in (31, 32, 33, 63, 64, 65)]               # a row that ends on, one before and one after a segment's end
LINES = [(1, 1, 16384), (1, 16384, 1)]
CONTENTS = ['one', 'blobs', 'noise', 'dots', 'corner', 'rim', 'hstripes', 'vstripes', 'last', 'absent']
MODES = [(None, False), (None, True), (0, False), (3, False), (255, False)]          # (value, border)
BRUTE_PIXELS = 300                                                   # frames up to this many pixels: the brute-force restatement


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _content(shape, content):
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    y, x = np.mgrid[0:H, 0:W]
    a = np.zeros(shape, dtype=np.uint8)
    if content == 'one':                                             # one value everywhere
        a[:] = 3
    elif content == 'blobs':
        a = census_ref.blobs(H * W + n, n, H, W)
    elif content == 'noise':
        a = rng.integers(0, 4, shape).astype(np.uint8)
    elif content == 'dots':                                          # one-pixel objects
        hit = (y % 4 == 1) & (x % 5 == 2)
        a[:, hit] = (1 + (y + x) % 3).astype(np.uint8)[hit]
        a[:, H // 2, W // 2] = 3
    elif content == 'corner':                                        # a single site in the last corner
        a[:, H - 1, W - 1] = 3
    elif content == 'rim':                                           # one object filling the frame but for a one-pixel rim
        a[:, 1:-1, 1:-1] = 3
    elif content == 'hstripes':
        a[:] = (y % 2 * 3).astype(np.uint8)
    elif content == 'vstripes':
        a[:] = (x % 2 * 3).astype(np.uint8)
    elif content == 'last':                                          # objects on the last row, the last column and the corner
        a[:, H - 1, :(W + 1) // 2] = 1
        a[:, :(H + 1) // 2, W - 1] = 2
        a[:, H - 1, W - 1] = 3
    elif content == 'absent':                                        # 0, 3 and 255 absent from even frames, present in odd ones
        a = rng.integers(1, 3, shape).astype(np.uint8)
        a[1::2] = np.array([0, 3, 255, 1], dtype=np.uint8)[rng.integers(0, 4, a[1::2].shape)]
    elif content == 'site0':                                         # a single site at flat index 0
        a[0, 0, 0] = 3
    else:
        raise KeyError(content)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(shape, content, mode):
    a = _content(shape, content)
    ref = R.brute if shape[1] * shape[2] <= BRUTE_PIXELS else R.edt
    d = ref(a, *mode)
    d.setflags(write=False)
    return d


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


def _tail_intact(t, size):
    return bool((t[size:] == CANARY32).all().item())


def _run_edt(dev, a, mode, offset=0):
    """rmem_label_edt on a guarded copy of a; dist2 and the workspace dirtied and followed by guard ints"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = a.shape
    value, border = mode
    stream = torch.cuda.current_stream(dev).cuda_stream
    buf, view, front = _guarded(dev, a, offset)
    need = int(L.rmem_label_edt_workspace_bytes(n, H, W))
    assert need % 4 == 0 and need >= 2 * a.size
    dist2, ws = _dirty(dev, a.size), _dirty(dev, need // 4)
    _lib.check(L.rmem_label_edt(view.data_ptr(), n, H, W, -1 if value is None else value, int(border), dist2.data_ptr(), ws.data_ptr(), need,
                                stream), 'rmem_label_edt')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, a.size), 'guard bytes around the stack'
    assert np.array_equal(buf[front:front + a.size].cpu().numpy(), a.reshape(-1)), 'the stack is read only'
    assert _tail_intact(dist2, a.size) and _tail_intact(ws, need // 4), 'ints beyond dist2 or the workspace were written'
    return dist2[:a.size].cpu().numpy().reshape(a.shape)


def _run_peaks(dev, d2, keys, offset=0):
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = keys.shape
    stream = torch.cuda.current_stream(dev).cuda_stream
    buf, view, front = _guarded(dev, keys, offset)
    d = torch.from_numpy(np.array(d2)).to(dev)                       # a copy: the shared reference is read only
    need = int(L.rmem_label_edt_peaks_workspace_bytes(n))
    table, ws = _dirty(dev, n * 512), _dirty(dev, need // 4)
    _lib.check(L.rmem_label_edt_peaks(d.data_ptr(), view.data_ptr(), n, H, W, table.data_ptr(), ws.data_ptr(), need, stream),
               'rmem_label_edt_peaks')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, keys.size) and _tail_intact(table, n * 512) and _tail_intact(ws, need // 4)
    assert np.array_equal(d.cpu().numpy(), d2), 'dist2 is read only'
    return table[:n * 512].cpu().numpy().reshape(n, 256, 2)


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES + EDGES, ids=lambda s: 'x'.join(map(str, s)))
def test_transform(dev, shape, content):
    """both modes, both borders, the values 0, 3 and 255, the stack starting at a byte offset that changes from mode to mode"""
    a = _content(shape, content)
    for k, mode in enumerate(MODES):
        offset = OFFSETS[(k + len(content)) % 4]
        got, want = _run_edt(dev, a, mode, offset), _ref(shape, content, mode)
        assert np.array_equal(got, want), (content, mode, offset, np.argwhere(got != want)[:8])


def test_contents_are_what_they_claim():
    assert (_ref((2, 3, 5), 'one', (None, False)) == S).all()                        # the sentinel without border ...
    assert _ref((2, 3, 5), 'one', (None, True))[0].tolist() == [[1] * 5, [1, 4, 4, 4, 1], [1] * 5]     # ... the edge distance with it
    assert _ref((1, 150, 200), 'corner', (None, False))[0, 0, 0] == 149 ** 2 + 199 ** 2
    assert _ref((1, 150, 200), 'corner', (3, False))[0, 0, 0] == 149 ** 2 + 199 ** 2
    assert _ref((1, 150, 200), 'rim', (None, True)).max() == 74 ** 2                 # the deepest interior
    d = _ref((2, 37, 131), 'absent', (255, False))
    assert (d[0] == S).all() and d[1].min() == 0 and d[1].max() < S


@pytest.mark.parametrize('shape', [(2, 37, 131), (1, 40, 1100)], ids=['2x37x131', '1x40x1100'])
def test_every_byte_offset(dev, shape):
    for content in ('blobs', 'noise'):
        a = _content(shape, content)
        for mode in MODES[:4]:
            for offset in OFFSETS:
                assert np.array_equal(_run_edt(dev, a, mode, offset), _ref(shape, content, mode)), (content, mode, offset)


@pytest.mark.parametrize('shape', LINES, ids=['row of 16384', 'column of 16384'])
def test_longest_lines(dev, shape):
    """a single site at index 0: distances up to 16383^2, a full row image, a scan as long as the row"""
    a = _content(shape, 'site0')
    x2 = (np.arange(16384, dtype=np.int64) ** 2).astype(np.int32).reshape(shape)
    for mode in ((None, False), (3, False), (None, True)):
        got, want = _run_edt(dev, a, mode, 13), _ref(shape, 'site0', mode)
        assert np.array_equal(got, want), (mode, np.argwhere(got != want)[:8])
        if mode == (3, False):
            assert np.array_equal(want, x2)
        if mode == (None, True):
            assert (want == 1).all()


@pytest.mark.parametrize('content', CONTENTS)
def test_peaks(dev, content):
    """against the restatement, keyed by the labels and by another stack"""
    for shape in ((2, 3, 5), (3, 17, 33), (2, 37, 131), (1, 40, 1100)):
        a = _content(shape, content)
        other = np.ascontiguousarray(np.roll(_content(shape, 'noise'), 1, axis=2))
        for k, mode in enumerate(MODES[:4]):
            d2 = _ref(shape, content, mode)
            for keys in (a, other):
                got, want = _run_peaks(dev, d2, keys, OFFSETS[k]), R.peaks_fast(d2, keys)
                assert np.array_equal(got, want), (content, shape, mode, np.argwhere(got != want)[:8])
    small = _content((2, 3, 5), content)
    d2 = _ref((2, 3, 5), content, MODES[1])
    assert np.array_equal(R.peaks(d2, small), R.peaks_fast(d2, small))


def test_peaks_plateau_and_all_keys(dev):
    """many pixels attain the maximum: the first in raster order; all 256 key values in one 16 x 16 frame"""
    keys = np.zeros((2, 37, 131), dtype=np.uint8)
    keys[:, 5:30, 7:120] = 4
    d2 = np.where(keys == 4, 9, 2).astype(np.int32)
    d2[1, 20, 50] = S                                                # the sentinel is a distance like any other here
    got = _run_peaks(dev, d2, keys, 3)
    assert got[0, 0].tolist() == [2, 0] and got[0, 4].tolist() == [9, 5 * 131 + 7] and got[1, 4].tolist() == [S, 20 * 131 + 50]
    assert np.array_equal(got, R.peaks(d2, keys))
    rng = np.random.default_rng(5)
    keys = rng.permutation(256).astype(np.uint8).reshape(1, 16, 16)
    d2 = rng.integers(0, 1 << 30, (1, 16, 16)).astype(np.int32)
    got = _run_peaks(dev, d2, keys, 1)
    assert (got[0, :, 0] >= 0).all() and np.array_equal(got, R.peaks(d2, keys))
    assert np.array_equal(got[0, keys.reshape(-1), 1], np.arange(256))


def test_python_functions_and_side_stream(dev):
    """label_edt and peaks through the package: [H, W] as one frame, out=, border ignored with a value; on a side stream, twice,
    byte-identical"""
    from rmem_ocu_amd import distance
    shape = (3, 17, 33)
    a = _content(shape, 'blobs')
    d = torch.from_numpy(a.copy()).to(dev)
    for mode in MODES:
        got = distance.label_edt(d, *mode)
        assert got.dtype == torch.int32 and got.shape == d.shape and np.array_equal(got.cpu().numpy(), _ref(shape, 'blobs', mode))
    one = distance.label_edt(d[1], 0, border=True)                   # border is ignored with a value
    assert one.shape == (17, 33) and np.array_equal(one.cpu().numpy(), _ref(shape, 'blobs', (0, False))[1])
    out = torch.full(shape, CANARY32, dtype=torch.int32, device=dev)
    assert distance.label_edt(d, out=out) is out and np.array_equal(out.cpu().numpy(), _ref(shape, 'blobs', (None, True)))
    table = distance.peaks(out, d)
    assert table.dtype == torch.int32 and table.shape == (3, 256, 2)
    assert np.array_equal(table.cpu().numpy(), R.peaks_fast(_ref(shape, 'blobs', (None, True)), a))
    assert distance.peaks(out[0], d[0]).shape == (1, 256, 2)
    from rmem_ocu_amd._lib import RmemError
    with pytest.raises(RmemError, match='out must be a contiguous int32 tensor'):
        distance.label_edt(d, out=out[:2])
    with pytest.raises(RmemError, match='dist2 must be an int32 tensor'):
        distance.peaks(out.float(), d)
    with pytest.raises(RmemError, match='one shape'):
        distance.peaks(out[:2], d)
    big = (2, 37, 131)
    b = torch.from_numpy(_content(big, 'noise').copy()).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs = [(distance.label_edt(b, None, False), distance.peaks(distance.label_edt(b, 3), b)) for _ in range(2)]
    side.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][0].cpu().numpy(), _ref(big, 'noise', (None, False)))
    assert np.array_equal(runs[0][1].cpu().numpy(), R.peaks_fast(_ref(big, 'noise', (3, False)), _content(big, 'noise')))


def _moved(a, dy, dx):
    b = np.zeros_like(a)
    b[:, dy:, dx:] = a[:, :a.shape[1] - dy, :a.shape[2] - dx]
    return b


def test_hausdorff(dev):
    from rmem_ocu_amd import _lib, distance
    from rmem_ocu_amd.evaluator import surface_distance
    shape = (3, 37, 131)
    a = census_ref.blobs(11, *shape)
    b = _moved(a, 2, 3)                                              # the blobs against themselves moved by (2, 3)
    b[1][b[1] == 2] = 0                                              # object 2 absent on one side of frame 1 ...
    a2 = a.copy()
    a2[a2 == 7] = 0
    b[b == 7] = 0                                                    # ... and object 7 on both
    da, db = torch.from_numpy(a2).to(dev), torch.from_numpy(b).to(dev)
    want = R.hausdorff2(a2, b, 10)
    assert (want[:, 6] == 0).all() and want[1, 1] == S and want[0, 2] == 13
    got = distance.hausdorff2(da, db, 10)
    assert got.dtype == torch.int32 and got.shape == (3, 10) and np.array_equal(got.cpu().numpy(), want)
    assert (distance.hausdorff2(da, da, 10) == 0).all()             # identical stacks
    L = _lib.lib()
    one = 37 * 131 * 4 + int(L.rmem_label_edt_workspace_bytes(1, 37, 131)) + 2 * int(L.rmem_label_edt_peaks_workspace_bytes(1))
    assert np.array_equal(distance.hausdorff2(da, db, 10, workspace_bytes=one).cpu().numpy(), want)          # one frame per pass
    assert np.array_equal(distance.hausdorff2(da, db, 10, workspace_bytes=2 * one + 1).cpu().numpy(), want)  # 2 + 1
    with pytest.raises(_lib.RmemError, match='workspace_bytes'):
        distance.hausdorff2(da, db, 10, workspace_bytes=one - 1)
    h = distance.hausdorff(da, db, 10)
    assert h.dtype == np.float64 and np.array_equal(h, np.where(want == S, np.inf, np.sqrt(want.astype(np.float64))))
    assert np.isinf(h[1, 1]) and np.array_equal(surface_distance(da, db, 10), h)
    assert np.array_equal(distance.hausdorff2(da[0], db[0], 3).cpu().numpy(), want[:1, :3])
    far = np.zeros((1, 40, 60), dtype=np.uint8)                      # a lone far pixel: J stays at 400 / 401, the distance does not
    far[0, 2:22, 2:22] = 1
    lone = far.copy()
    lone[0, 39, 59] = 1
    got = distance.hausdorff2(torch.from_numpy(far).to(dev), torch.from_numpy(lone).to(dev), 1).cpu().numpy()
    assert got.tolist() == [[18 ** 2 + 38 ** 2]] and np.array_equal(got, R.hausdorff2(far, lone, 1))


def test_next_clicks(dev):
    from rmem_ocu_amd.evaluator import next_clicks

    def run(pred, gt, k):
        got = next_clicks(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), k)
        assert got.dtype == np.int32 and got.shape == (pred.shape[0], k, 4)
        assert np.array_equal(got, R.next_clicks(pred, gt, k)), (got, R.next_clicks(pred, gt, k))
        return got.tolist()

    gt = np.zeros((1, 5, 7), dtype=np.uint8)
    gt[0, 1:4, 1:4] = 1
    pred = np.zeros_like(gt)
    assert run(gt, gt, 1) == [[[-1, -1, 0, 0]]]                      # pred == gt
    assert run(pred, gt, 1) == [[[2, 2, 1, 4]]]                      # only false negatives
    assert run(gt, pred, 1) == [[[2, 2, 0, 4]]]                      # only false positives
    pred[0, 1:4, 4:7] = 1
    assert run(pred, gt, 1) == [[[2, 5, 0, 4]]]                      # equal depths: the false positive
    pred[:] = 0
    pred[0, 3:5, 4:7] = 1                                            # an error on the frame's edge: the border rule keeps it at depth 1
    assert run(pred, gt, 1) == [[[2, 2, 1, 4]]]
    assert run(pred, np.zeros_like(gt), 1) == [[[3, 4, 0, 1]]]
    shape = (2, 37, 131)
    a = census_ref.blobs(12, *shape)
    run(_moved(a, 3, 2), a, 10)                                      # 10 objects against the restatement
