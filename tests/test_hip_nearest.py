"""The nearest-site feature transform of label stacks on the MI355X against tests/nearest_ref.py: exact integer equality of whole
arrays, no tolerance.  The stack sits between guard bytes and starts at any byte, outputs and workspace are dirtied first and
followed by guards.  The shapes are test_hip_edt.py's, the smallest that can go wrong: one pixel, one row, one column, rows longer
than a workgroup's stride and than several column segments, columns taller than any band, and the two 16384-long lines.  What is
new against the distance transform is the TIE RULE (among equally near sites the smallest flat index): dots and stripes are full of
ties, and the frames written out by hand catch a scan that stops or skips a segment at dx^2 == best instead of above it.  The keys
of a (shape, content, site set) are computed once and shared by every limit, fill set and test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import census_ref
import nearest_ref as R

pytestmark = pytest.mark.gpu

S = R.SENTINEL
CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 3, 5), (3, 17, 33), (2, 37, 131), (1, 40, 1100), (1, 1100, 40), (1, 150, 200)]
EDGES = [(2, 3, W) for W in (31, 32, 33, 63, 64, 65)]               # a row that ends on, one before and one after a segment's end
LINES = [(1, 1, 16384), (1, 16384, 1)]
CONTENTS = ['one', 'blobs', 'noise', 'dots', 'corner', 'rim', 'hstripes', 'vstripes', 'last', 'absent']
SITE_SETS = [(3,), (1, 2, 3), (0,), (255,), ()]
FILLS = [None, (0,), (0, 255), (0, 1, 3)]                            # None: every value
LIMITS = (-1, 0, 2, 5)
BRUTE_PIXELS = 300                                                   # frames up to this many pixels: the brute-force restatement
ALL = (True, True, True)                                             # (index, dist2, taken) asked for


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
    elif content == 'dots':                                          # one-pixel objects on a grid: ties everywhere
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
    elif content == 'site0+16382':                                   # two sites on a line: the pixel at 8191 is as far from either
        a.reshape(-1)[[0, 16382]] = 3
    else:
        raise KeyError(content)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _keys(shape, content, sites):
    """the minima of (d2, index), once per stack and site set: every limit and fill set is derived from them (R.finish)"""
    a = _content(shape, content)
    site = np.isin(a, list(sites)).reshape(shape[0], -1)
    if shape[1] * shape[2] <= BRUTE_PIXELS:
        k = R.brute_keys(a, sites)
    elif site.sum(axis=1).max() <= 2:
        k = R.sparse_keys(a, sites)
    else:
        k = R.separable_keys(a, sites, bound=True)
    k.setflags(write=False)
    return k


def _ref(shape, content, sites, fill=None, max_d2=-1):
    return R.finish(_content(shape, content), _keys(shape, content, tuple(sites)), fill, max_d2)


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _words(values):
    return None if values is None else (ctypes.c_uint * 8)(*R.bits(values))


def _run(dev, a, sites, fill=None, limits=(-1,), offset=0, outs=ALL):
    """rmem_label_nearest on a guarded copy of a, once per limit; the outputs asked for and the workspace dirtied and followed by
    guards; one synchronise -> [(index, dist2, taken) per limit], None for an output not asked for"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = a.shape
    m, size = len(limits), a.size
    stream = torch.cuda.current_stream(dev).cuda_stream
    buf, view, front = _guarded(dev, a, offset)
    need = int(L.rmem_label_nearest_workspace_bytes(n, H, W))
    assert need % 4 == 0 and need >= 2 * size
    index, dist2, ws = (torch.full((k + 64,), CANARY32, dtype=torch.int32, device=dev) for k in (m * size, m * size, need // 4))
    taken = torch.full((m * size + 64,), CANARY, dtype=torch.uint8, device=dev)
    for k, max_d2 in enumerate(limits):
        ptr = [t[k * size:].data_ptr() if want else None for t, want in zip((index, dist2, taken), outs)]
        _lib.check(L.rmem_label_nearest(view.data_ptr(), n, H, W, _words(sites), _words(fill), max_d2, ptr[0], ptr[1], ptr[2], ws.data_ptr(),
                                        need, stream), 'rmem_label_nearest')
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:front] == CANARY).all() and (h[front + size:] == CANARY).all(), 'guard bytes around the stack'
    assert np.array_equal(h[front:front + size], a.reshape(-1)), 'the stack is read only'
    host = [index.cpu().numpy(), dist2.cpu().numpy(), taken.cpu().numpy()]
    for t, want, canary in zip(host, outs, (CANARY32, CANARY32, CANARY)):
        assert (t[m * size if want else 0:] == canary).all(), 'beyond an output, or an output not asked for, was written'
    assert (ws[need // 4:] == CANARY32).all().item(), 'ints beyond the workspace were written'
    return [tuple(t[k * size:(k + 1) * size].reshape(a.shape) if want else None for t, want in zip(host, outs)) for k in range(m)]


def _same(got, want):
    return all(g is None or np.array_equal(g, w) for g, w in zip(got, want))


def _where(got, want):
    return [np.argwhere(g != w)[:4].tolist() for g, w in zip(got, want) if g is not None]


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES + EDGES, ids=lambda s: 'x'.join(map(str, s)))
def test_transform(dev, shape, content):
    """every site set and every limit, all three outputs; the fill set and the byte offset of the stack change from set to set"""
    a = _content(shape, content)
    for k, sites in enumerate(SITE_SETS):
        fill, offset = FILLS[(k + len(content)) % 4], OFFSETS[(k + len(content)) % 4]
        for max_d2, got in zip(LIMITS, _run(dev, a, sites, fill, LIMITS, offset)):
            want = _ref(shape, content, sites, fill, max_d2)
            assert _same(got, want), (content, sites, fill, max_d2, offset, _where(got, want))


def test_contents_are_what_they_claim():
    index, dist2, _ = _ref((1, 150, 200), 'corner', (3,))
    assert (index == 150 * 200 - 1).all() and dist2[0, 0, 0] == 149 ** 2 + 199 ** 2
    index, dist2, taken = _ref((2, 37, 131), 'absent', (255,), (1, 2))
    assert (index[0] == -1).all() and (dist2[0] == S).all() and (index[1] >= 0).all() and (taken[1] == 255).sum() > (taken[0] == 255).sum() == 0
    index, dist2, _ = _ref((3, 17, 33), 'dots', (1, 2, 3))
    a = _content((3, 17, 33), 'dots')
    ties = 0                                                         # pixels with more than one nearest site: the rule decides them
    site = np.argwhere(a[0] > 0)
    for y, x in np.ndindex(17, 33):
        ties += int((((site - (y, x)) ** 2).sum(axis=1) == dist2[0, y, x]).sum() > 1)
    assert ties > 50
    assert (_ref((2, 3, 5), 'noise', ())[0] == -1).all()
    index, dist2, _ = _ref((2, 37, 131), 'blobs', (1, 2, 3), None, 5)
    assert (dist2[index >= 0] <= 5).all() and (index < 0).any() and (index >= 0).any()


@pytest.mark.parametrize('shape', [(2, 37, 131), (1, 40, 1100)], ids=['2x37x131', '1x40x1100'])
def test_every_byte_offset(dev, shape):
    for content, sites in (('blobs', (1, 2, 3)), ('noise', (3,)), ('dots', (1, 2, 3))):
        a = _content(shape, content)
        for offset in OFFSETS:
            for max_d2, got in zip((-1, 5), _run(dev, a, sites, (0,), (-1, 5), offset)):
                assert _same(got, _ref(shape, content, sites, (0,), max_d2)), (content, offset, max_d2)


@pytest.mark.parametrize('shape', LINES, ids=['row of 16384', 'column of 16384'])
def test_longest_lines(dev, shape):
    """a single site at index 0: offsets and distances up to 16383 and its square, a full row image in LDS, a scan as long as the
    row; sites at 0 and 16382: the pixel at 8191 is as far from either and goes to index 0"""
    line = np.arange(16384, dtype=np.int64)
    limits = (-1, 5, 8191 ** 2 - 1, 8191 ** 2, 2 ** 30)
    for content in ('site0', 'site0+16382'):
        a = _content(shape, content)
        for max_d2, got in zip(limits, _run(dev, a, (3,), (0,), limits, 13)):
            want = _ref(shape, content, (3,), (0,), max_d2)
            assert _same(got, want), (content, max_d2, _where(got, want))
    index, dist2, taken = _ref(shape, 'site0', (3,), (0,))
    assert (index == 0).all() and np.array_equal(dist2.reshape(-1), line ** 2) and (taken == 3).all()
    index, dist2, _ = _ref(shape, 'site0+16382', (3,), (0,))
    assert index.reshape(-1)[8191] == 0 and index.reshape(-1)[8192] == 16382 and dist2.reshape(-1)[8191] == 8191 ** 2
    index, _, taken = _ref(shape, 'site0+16382', (3,), (0,), 8191 ** 2 - 1)
    assert index.reshape(-1)[8191] == -1 and taken.reshape(-1)[8191] == 0 and (index >= 0).sum() == 16383


def test_tie_frames_written_out_by_hand(dev):
    for sites_at, pixel, want in R.TIES:
        a = R.tie_frame(sites_at)[None]
        (index, dist2, taken), = _run(dev, a, (3,), (0,))
        assert index[0][pixel] == want and taken[0][pixel] == 3, (sites_at, pixel, index)
        assert _same((index, dist2, taken), R.brute(a, (3,), (0,)))
    # the last pattern moved to the end of a column segment of 32: the same-row site lies in the NEXT segment (a segment skipped
    # at dx^2 + smallest^2 == best loses it), mirrored into the segment BEFORE, and two rows down, where the segment's smallest
    # offset is not zero
    for sites_at, pixel, want in ((((6, 31), (5, 32)), (5, 31), 5 * 70 + 32),
                                  (((5, 31), (6, 32)), (5, 32), 5 * 70 + 31),
                                  (((7, 31), (4, 32)), (5, 31), 4 * 70 + 32),       # d2 4 below against 1 + 1: the nearer wins
                                  (((7, 31), (5, 33)), (5, 31), 5 * 70 + 33),       # d2 4 against d2 4 in the next segment
                                  (((7, 32), (5, 30)), (5, 32), 5 * 70 + 30),       # and in the segment before
                                  (((3, 63), (7, 64)), (5, 63), 3 * 70 + 63),       # above in the own column stays against d2 5
                                  (((3, 64), (6, 63)), (5, 63), 6 * 70 + 63)):
        a = R.tie_frame(sites_at, (17, 70))[None]
        for limit in (-1, int(R.brute(a, (3,))[1][0][pixel])):       # without a limit, and with the limit at the winner's distance
            (index, dist2, taken), = _run(dev, a, (3,), None, (limit,))
            assert index[0][pixel] == want, (sites_at, pixel, limit, index[0][pixel])
            assert _same((index, dist2, taken), R.brute(a, (3,), None, limit))


def test_taken_and_fill(dev):
    """grow at r = 1, r = 2 and without a limit; a void value that is neither site nor fill stays; fill pixels that are sites map
    to themselves; only the pixels in fill change"""
    shape = (2, 37, 131)
    a = np.array(_content(shape, 'blobs'))
    a[:, 5:9, 60:90] = 255                                           # a void bar across whatever lies there
    objects = tuple(range(1, 11))
    for max_d2 in (1, 4, -1):
        (_, _, taken), = _run(dev, a, objects, (0,), (max_d2,), 3)
        want = R.separable(a, objects, (0,), max_d2, bound=True)[2]
        assert np.array_equal(taken, want)
        assert np.array_equal(taken[a != 0], a[a != 0]) and (taken == 255).sum() == (a == 255).sum()      # objects and void untouched
        assert ((taken != 0) & (a == 0)).any() and ((max_d2 >= 0) == bool((taken == 0).any()))
    (index, _, taken), = _run(dev, a, (0,) + objects, (0, 255), (-1,), 1)               # the background is a site AND in fill
    assert np.array_equal(taken[a == 0], a[a == 0]) and (taken != 255).all()
    assert np.array_equal(index[a != 255], np.broadcast_to(np.arange(37 * 131).reshape(37, 131), shape)[a != 255])
    assert _same((index, None, taken), R.separable(a, (0,) + objects, (0, 255), -1, bound=True))


def test_every_combination_of_outputs(dev):
    """an output that is not asked for is not written, and those asked for do not depend on the others: the taken-only call, which
    copies pixels outside fill without a scan and leaves rows without a fill pixel early, equals the taken of the full call"""
    for shape, content, sites, fill in (((2, 37, 131), 'blobs', (1, 2, 3), (0,)), ((3, 17, 33), 'dots', (1, 2, 3), (0, 3)),
                                        ((2, 37, 131), 'absent', (255,), (1,)), ((1, 40, 1100), 'last', (1, 2, 3), (0,)),
                                        ((3, 17, 33), 'rim', (0,), (3,)), ((2, 3, 5), 'noise', (), None)):
        a = _content(shape, content)
        for mask in range(1, 8):
            outs = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
            for max_d2, got in zip((-1, 2), _run(dev, a, sites, fill, (-1, 2), OFFSETS[mask % 4], outs)):
                assert [g is not None for g in got] == list(outs)
                assert _same(got, _ref(shape, content, sites, fill, max_d2)), (content, outs, max_d2)


def test_singleton_site_sets_equal_label_edt(dev):
    from rmem_ocu_amd import distance
    for shape, content in (((2, 37, 131), 'blobs'), ((3, 17, 33), 'noise'), ((2, 37, 131), 'absent'), ((1, 40, 1100), 'dots')):
        d = torch.from_numpy(_content(shape, content).copy()).to(dev)
        for v in (0, 3, 255):
            index, dist2 = distance.nearest(d, (v,))
            assert torch.equal(dist2, distance.label_edt(d, v)), (content, v)
            assert torch.equal(index >= 0, dist2 != S)


def test_python_functions_and_side_stream(dev):
    """nearest and grow through the package: [H, W] as one frame, max_distance against max_d2, return_distance, out=; on a side
    stream, twice, byte-identical"""
    from rmem_ocu_amd import distance
    from rmem_ocu_amd._lib import RmemError
    shape = (3, 17, 33)
    a = _content(shape, 'blobs')
    d = torch.from_numpy(a.copy()).to(dev)
    index, dist2 = distance.nearest(d, [1, 2, 3])
    assert index.dtype == dist2.dtype == torch.int32 and index.shape == dist2.shape == d.shape
    assert _same((index.cpu().numpy(), dist2.cpu().numpy()), _ref(shape, 'blobs', (1, 2, 3)))
    index, none = distance.nearest(d[1], {1, 2, 3}, max_distance=2.3, return_distance=False)             # int(2.3 * 2.3) = 5
    assert none is None and index.shape == (17, 33) and np.array_equal(index.cpu().numpy(), _ref(shape, 'blobs', (1, 2, 3), None, 5)[0][1])
    assert torch.equal(distance.nearest(d, (3,), max_d2=5)[1], distance.nearest(d, (3,), max_distance=2.3)[1])
    grown = distance.grow(d, max_distance=2)                                                             # fill (0,), sites: the rest
    assert grown.dtype == torch.uint8 and grown.shape == d.shape
    assert np.array_equal(grown.cpu().numpy(), R.brute(a, range(1, 256), (0,), 4)[2]) and not torch.equal(grown, d)
    assert np.array_equal(distance.grow(d[2], fill=(0, 5), sites=(1, 2)).cpu().numpy(), R.brute(a[2], (1, 2), (0, 5))[2])
    out = torch.full(shape, CANARY, dtype=torch.uint8, device=dev)
    assert distance.grow(d, out=out) is out and np.array_equal(out.cpu().numpy(), R.brute(a, range(1, 256), (0,))[2])
    assert torch.equal(d.cpu(), torch.from_numpy(a.copy()))
    with pytest.raises(RmemError, match='out must be a contiguous uint8 tensor'):
        distance.grow(d, out=out[:2])
    with pytest.raises(RmemError, match='out must not be the labels'):
        distance.grow(d, out=d)
    big = (2, 37, 131)
    b = torch.from_numpy(_content(big, 'dots').copy()).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs = [distance.nearest(b, (1, 2, 3)) + (distance.grow(b),) for _ in range(2)]
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert _same([t.cpu().numpy() for t in runs[0]], _ref(big, 'dots', (1, 2, 3), (0,)))


def test_evaluator_wrappers(dev):
    from rmem_ocu_amd.evaluator import expand_masks, fill_void, labels_from_seeds
    a = np.zeros((2, 9, 12), dtype=np.uint8)
    a[:, 2:7, 1:5] = 1                                               # two blobs one gap apart ...
    a[:, 2:7, 6:10] = 2
    a[1, 4, 5] = 255                                                 # ... and a void pixel in the gap of frame 1
    d = torch.from_numpy(a).to(dev)
    got = expand_masks(d, 1).cpu().numpy()
    assert np.array_equal(got, R.brute(a, range(1, 256), (0,), 1)[2])
    assert (got[0, 2:7, 5] == 1).all()                               # the gap is as far from either: the site first in raster order
    assert np.array_equal(got[a != 0], a[a != 0])                    # objects never overwrite each other
    assert (got[0, 1, 1:5] == 1).all() and (got[0, 1, 6:10] == 2).all() and got[0, 1, 5] == 0 and got[0, 0].max() == 0
    assert got[1, 3, 5] == 1 and got[1, 4, 5] == 255                 # without void=, 255 is an object like any other ...
    wide = expand_masks(d, 2, void=255).cpu().numpy()                # ... with it, it is neither filled nor spread
    assert np.array_equal(wide, R.brute(a, range(1, 255), (0,), 4)[2]) and wide[1, 4, 5] == 255 and (wide[1, 2:7, 5] != 2).all()
    assert np.array_equal(expand_masks(d, 2).cpu().numpy(), R.brute(a, range(1, 256), (0,), 4)[2])
    assert expand_masks(d[0], 1).shape == (9, 12) and torch.equal(expand_masks(d, 0), d)
    rim = np.array(_content((2, 37, 131), 'blobs'))
    for v in range(1, 11):                                           # a void rim round every blob
        m = rim == v
        inner = m & np.roll(m, 1, 1) & np.roll(m, -1, 1) & np.roll(m, 1, 2) & np.roll(m, -1, 2)
        rim[m & ~inner] = 255
    r = torch.from_numpy(rim).to(dev)
    filled = fill_void(r).cpu().numpy()
    assert np.array_equal(filled, R.separable(rim, [v for v in range(256) if v != 255], (255,), -1, bound=True)[2])
    assert (filled != 255).all() and np.array_equal(filled[rim != 255], rim[rim != 255])
    near = fill_void(r, max_distance=1).cpu().numpy()
    assert np.array_equal(near, R.separable(rim, [v for v in range(256) if v != 255], (255,), 1, bound=True)[2])
    assert np.array_equal(fill_void(d, void=2).cpu().numpy(), R.brute(a, [v for v in range(256) if v != 2], (2,))[2])
    void = torch.full((1, 5, 7), 255, dtype=torch.uint8, device=dev)
    assert torch.equal(fill_void(void), void)                        # nothing but void: as it is
    seeds = np.zeros((2, 17, 33), dtype=np.uint8)                    # frame 1 has no seed
    seeds[0, 3, 4], seeds[0, 12, 20], seeds[0, 8, 30], seeds[0, 3:6, 14] = 1, 2, 9, 1
    s = torch.from_numpy(seeds).to(dev)
    lab = labels_from_seeds(s).cpu().numpy()
    want = R.brute(seeds, range(1, 256), (0,))[2]
    assert np.array_equal(lab, want) and (lab[0] != 0).all() and np.array_equal(lab[1], seeds[1])
    neg = labels_from_seeds(s, background=9).cpu().numpy()           # the seed of value 9 claims its region, which is then background
    assert np.array_equal(neg, np.where(want == 9, 0, want)) and (neg[0] == 0).sum() == (want[0] == 9).sum() > 0
    assert np.array_equal(labels_from_seeds(s, max_distance=3).cpu().numpy(), R.brute(seeds, range(1, 256), (0,), 9)[2])
    assert torch.equal(labels_from_seeds(s[1]), s[1])
