"""The surface metrics of label stacks on the MI355X against tests/surface_ref.py: exact integer equality on whole arrays, and the
float metrics within the bounds their arithmetic gives.  Stacks sit between guard bytes and start at any byte, outputs are dirtied
first and followed by guards.  The shapes are the smallest that can go wrong: one pixel, one row, one column, rows longer than a
workgroup's stride, the two 16384-long lines, and samples that differ only in one digit of the census' radix select.  Contents and
references are computed once per case and shared (contents and guards are those of test_hip_edt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import census_ref
import surface_ref as R
from test_hip_edt import CANARY, CANARY32, EDGES, OFFSETS, _content, _dirty, _guarded, _guards_intact, _moved, _tail_intact

pytestmark = pytest.mark.gpu

S = R.SENTINEL
CANARY64 = int(np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0])
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 3, 5), (3, 17, 33), (2, 37, 131), (1, 40, 1100)]
CONTENTS = ['one', 'blobs', 'noise', 'dots', 'rim', 'hstripes', 'vstripes', 'last']
IDS = dict(ids=lambda s: 'x'.join(map(str, s)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _lib():
    from rmem_ocu_amd import _lib
    return _lib, _lib.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _run_surface(dev, a, offset, out_offset):
    """rmem_label_surface on a guarded copy of a into a guarded, dirtied output, each at its own byte offset"""
    lib, L = _lib()
    n, H, W = a.shape
    buf, view, front = _guarded(dev, a, offset)
    obuf, oview, ofront = _guarded(dev, np.full(a.shape, CANARY, dtype=np.uint8), out_offset)
    lib.check(L.rmem_label_surface(view.data_ptr(), n, H, W, oview.data_ptr(), _stream(dev)), 'rmem_label_surface')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, a.size) and _guards_intact(obuf, ofront, a.size), 'guard bytes around the stacks'
    assert np.array_equal(buf[front:front + a.size].cpu().numpy(), a.reshape(-1)), 'the stack is read only'
    return oview.cpu().numpy()


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, **IDS)
def test_surface(dev, shape, content):
    a = _content(shape, content)
    want = R.surface(a)
    for k, offset in enumerate(OFFSETS):
        got = _run_surface(dev, a, offset, OFFSETS[(k + len(content)) % 4])
        assert np.array_equal(got, want), (content, offset, np.argwhere(got != want)[:8])


def test_surfaces_are_what_they_claim(dev):
    assert np.array_equal(R.surface(_content((2, 3, 5), 'one')), [[[3] * 5, [3, 0, 0, 0, 3], [3] * 5]] * 2)
    rim = R.surface(_content((3, 17, 33), 'rim'))[0]                 # the rim is background on the frame's edge; the object keeps a ring
    assert (rim[0] == 0).all() and (rim[1, 1:-1] == 3).all() and (rim[2:-2, 2:-2] == 0).all()
    from rmem_ocu_amd import surface
    a = _content((2, 37, 131), 'blobs')
    d = torch.from_numpy(a.copy()).to(dev)
    got = surface.label_surface(d)
    assert got.dtype == torch.uint8 and got.shape == d.shape and np.array_equal(got.cpu().numpy(), R.surface(a))
    assert surface.label_surface(d[1]).shape == (37, 131)


def _run_at(dev, labels, keys, value, key, offset=0):
    """rmem_label_edt_at on guarded copies; samples and the workspace dirtied and followed by guard ints -> samples"""
    lib, L = _lib()
    n, H, W = labels.shape
    buf, view, front = _guarded(dev, labels, offset)
    kbuf, kview, kfront = _guarded(dev, keys, OFFSETS[(OFFSETS.index(offset) + 1) % 4])
    need = int(L.rmem_label_edt_workspace_bytes(n, H, W))
    samples, ws = _dirty(dev, labels.size), _dirty(dev, need // 4)
    lib.check(L.rmem_label_edt_at(view.data_ptr(), kview.data_ptr(), n, H, W, value, key, samples.data_ptr(), ws.data_ptr(), need, _stream(dev)),
              'rmem_label_edt_at')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, labels.size) and _guards_intact(kbuf, kfront, keys.size), 'guard bytes around the stacks'
    assert _tail_intact(samples, labels.size) and _tail_intact(ws, need // 4), 'ints beyond samples or the workspace were written'
    return samples[:labels.size].cpu().numpy().reshape(labels.shape)


@functools.lru_cache(maxsize=None)
def _full(shape, content, value):
    """distance.label_edt(labels, value) on the device: what the sampled transform must equal on the key pixels"""
    from rmem_ocu_amd import distance
    d = distance.label_edt(torch.from_numpy(_content(shape, content).copy()).cuda(0), value).cpu().numpy()
    d.setflags(write=False)
    return d


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES + EDGES, **IDS)
def test_edt_at(dev, shape, content):
    """keys in the stack itself and in another one; a key and a value that no pixel holds"""
    a = _content(shape, content)
    other = np.ascontiguousarray(np.roll(_content(shape, 'noise'), 1, axis=2))
    for k, (value, key, keys) in enumerate(((3, 0, a), (0, 3, a), (3, 3, a), (3, 2, other), (1, 3, other), (3, 77, a), (77, 3, a), (77, 0, other))):
        got = _run_at(dev, a, keys, value, key, OFFSETS[(k + len(content)) % 4])
        on = keys == key
        assert (got[~on] == CANARY32).all(), (content, value, key, 'an entry off the key was written')
        want = _full(shape, content, value)
        assert np.array_equal(got[on], want[on]), (content, value, key, np.argwhere(on & (got != want))[:8])
        if value == 77:
            assert (got[on] == S).all()
        if key == 77:
            assert not on.any()


@pytest.mark.parametrize('shape', [(1, 1, 16384), (1, 16384, 1)], ids=['row of 16384', 'column of 16384'])
def test_edt_at_longest_lines(dev, shape):
    """one site at index 0, one key pixel at the far end: the largest distance, a full row image in LDS, a scan as long as the row"""
    a = _content(shape, 'site0')
    keys = np.zeros(shape, dtype=np.uint8)
    keys.reshape(-1)[-1] = 5
    got = _run_at(dev, a, keys, 3, 5, 13).reshape(-1)
    assert got[-1] == 16383 ** 2 and (got[:-1] == CANARY32).all()
    every = _run_at(dev, a, np.full(shape, 5, dtype=np.uint8), 3, 5, 1).reshape(-1)       # every pixel a key pixel
    assert np.array_equal(every, (np.arange(16384, dtype=np.int64) ** 2).astype(np.int32))


def test_edt_at_python_and_side_stream(dev):
    from rmem_ocu_amd import surface
    from rmem_ocu_amd._lib import RmemError
    shape = (2, 37, 131)
    a, want = _content(shape, 'noise'), _full(shape, 'noise', 3)
    d = torch.from_numpy(a.copy()).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    runs = []
    with torch.cuda.stream(side):
        for _ in range(2):
            samples = torch.full(shape, CANARY32, dtype=torch.int32, device=dev)
            assert surface.edt_at(d, d, 3, 1, samples) is samples
            runs.append(samples)
    side.synchronize()
    assert torch.equal(runs[0], runs[1])
    got = runs[0].cpu().numpy()
    assert np.array_equal(got[a == 1], want[a == 1]) and (got[a != 1] == CANARY32).all()
    one = torch.full((37, 131), CANARY32, dtype=torch.int32, device=dev)
    assert np.array_equal(surface.edt_at(d[1], d[1], 3, 1, one).cpu().numpy(), got[1])
    with pytest.raises(RmemError, match='samples must be a contiguous int32 tensor'):
        surface.edt_at(d, d, 3, 1, runs[0][:1])
    with pytest.raises(RmemError, match='one shape'):
        surface.edt_at(d, d[:1], 3, 1, runs[0])


# ------------------------------------------------------------------------------------------------------------------ census
def _run_census(dev, da, sa, db, sb, K, tol2=(), q=9500, offset=0):
    """rmem_surface_census on reference samples and surfaces: entries off the surfaces hold garbage, the table and the workspace are
    dirtied and followed by guards"""
    lib, L = _lib()
    n, H, W = sa.shape
    bufs = [_guarded(dev, s, o) for s, o in ((sa, offset), (sb, OFFSETS[(OFFSETS.index(offset) + 2) % 4]))]
    dd = [torch.from_numpy(np.where(d < 0, CANARY32, d).astype(np.int32)).to(dev) for d in (da, db)]
    need = int(L.rmem_surface_census_workspace_bytes(n, K))
    assert need % 8 == 0
    table = torch.full((n * K * 27 + 64,), CANARY64, dtype=torch.int64, device=dev)
    ws = torch.full((need // 8 + 64,), CANARY64, dtype=torch.int64, device=dev)
    tol = (ctypes.c_int * 4)(*tol2)
    lib.check(L.rmem_surface_census(dd[0].data_ptr(), bufs[0][1].data_ptr(), dd[1].data_ptr(), bufs[1][1].data_ptr(), n, H, W, K, tol, len(tol2), q,
                                    table.data_ptr(), ws.data_ptr(), need, _stream(dev)), 'rmem_surface_census')
    torch.cuda.synchronize()
    for (buf, _, front), s in zip(bufs, (sa, sb)):
        assert _guards_intact(buf, front, s.size), 'guard bytes around the surface stacks'
    assert bool((table[n * K * 27:] == CANARY64).all()) and bool((ws[need // 8:] == CANARY64).all()), 'beyond the table or the workspace'
    return table[:n * K * 27].cpu().numpy().reshape(n, K, 3, 9)


def _check_census(dev, a, b, K, tol2=(), q=9500, offset=0):
    want = R.census(a, b, K, tol2, q)
    da, db = R.samples_edt(a, b, K)
    got = _run_census(dev, da, R.surface(a), db, R.surface(b), K, tol2, q, offset)
    assert np.array_equal(got, want), (K, tol2, q, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return want


@functools.lru_cache(maxsize=None)
def _pair(shape):
    """blobs against themselves moved by (2, 3); object 2 absent on one side of the last frame, object 7 on both sides everywhere"""
    a = census_ref.blobs(11, *shape).copy()
    b = _moved(a, 2, 3)
    b[-1][b[-1] == 2] = 0
    a[a == 7] = 0
    b[b == 7] = 0
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@pytest.mark.parametrize('shape', [(2, 3, 5), (3, 17, 33), (2, 37, 131)], **IDS)
def test_census_of_moved_blobs(dev, shape):
    a, b = _pair(shape)
    for k, (K, tol2, q) in enumerate(((10, (1, 4), 9500), (10, (), 5000), (3, (0, 1, 4, 2 ** 30 - 1), 0), (1, (9,), 10000), (10, (0,), 9500))):
        want = _check_census(dev, a, b, K, tol2, q, OFFSETS[k % 4])
        if K == 10:
            assert (want[:, 6, :, 0] == 0).all() and (want[:, 6, :, 2] == -1).all()           # absent on both sides: empty rows
    same = _check_census(dev, a, a, 10, (0, 1), 9500)                                     # identical stacks: every sample is 0
    assert (same[..., 1:5].max() == 0) and np.array_equal(same[..., 5], same[..., 0]) and np.array_equal(same[..., 6], same[..., 0])
    if shape == (2, 37, 131):
        assert want[-1, 1, 0, 2] == S or want[-1, 1, 1, 2] == S                           # absent on one side: a row of sentinels


def test_census_lone_far_pixel_and_255_objects(dev):
    far = np.zeros((1, 40, 60), dtype=np.uint8)
    far[0, 2:22, 2:22] = 1
    lone = far.copy()
    lone[0, 39, 59] = 1
    want = _check_census(dev, far, lone, 1, (1,), 9500, 3)
    assert want[0, 0, 2, 2] == 18 ** 2 + 38 ** 2 and want[0, 0, 2, 4] == 0                # the maximum sees it, the 95th percentile does not
    rng = np.random.default_rng(6)
    a = rng.permutation(256).astype(np.uint8).reshape(1, 16, 16)                         # every object 1..255 is one pixel
    b = np.ascontiguousarray(np.roll(a, (3, 5), axis=(1, 2)))
    want = _check_census(dev, a, b, 255, (0, 40), 9500, 1)
    assert (want[0, :, :2, 0] == 1).all() and (want[0, :, 2, 0] == 2).all()


ROWS = [(8, (3, 5, 7)), (64, (40, 45, 50)), (1100, (1030, 1050, 1090)), (16384, (16383,))]


@pytest.mark.parametrize('W,cols', ROWS, ids=['low digit', 'middle digit', 'high digit', '16383 squared'])
def test_census_digits(dev, W, cols):
    """one-row frames: object 1 of b is the pixel at x = 0 and object 1 of a sits at the given columns, so the samples are x^2 and
    differ only in the low bits, only in the middle, or only above 2^20"""
    a, b = np.zeros((1, 1, W), dtype=np.uint8), np.zeros((1, 1, W), dtype=np.uint8)
    a[0, 0, list(cols)] = 1
    b[0, 0, 0] = 1
    da, db = R.samples_edt(a, b, 1)
    assert sorted(da[a == 1].tolist()) == [c * c for c in cols] and db[0, 0, 0] == cols[0] ** 2
    for k, q in enumerate((0, 5000, 9500, 10000)):
        want = _check_census(dev, a, b, 1, (cols[0] ** 2, cols[-1] ** 2 - 1), q, OFFSETS[k])
        assert want[0, 0, 0, 2] == cols[-1] ** 2 and want[0, 0, 0, 3] == [c * c for c in cols][(len(cols) - 1) * q // 10000]


def test_census_plateau(dev):
    """all samples equal: lo = hi = max whatever the rank"""
    a, b = np.zeros((2, 5, 70), dtype=np.uint8), np.zeros((2, 5, 70), dtype=np.uint8)
    a[:, 0, :] = 1
    b[:, 3, :] = 1
    for q in (0, 5000, 9500, 10000):
        want = _check_census(dev, a, b, 1, (8, 9), q, 13)
        assert (want[:, 0, :, 2:5] == 9).all() and want[0, 0, 2].tolist()[5:] == [0, 140, 0, 0]


def test_surface_census_through_the_package(dev):
    """surfaces, sampled transforms and census in one call; one frame per pass against the whole stack"""
    from rmem_ocu_amd import surface
    from rmem_ocu_amd._lib import RmemError
    shape = (3, 17, 33)
    a, b = _pair(shape)
    da, db = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    want = R.census(a, b, 10, (1, 4), 9500)
    got = surface.surface_census(da, db, 10, (1, 4))
    assert got.dtype == torch.int64 and got.shape == (3, 10, 3, 9) and np.array_equal(got.cpu().numpy(), want)
    lib, L = _lib()
    one = int(L.rmem_surface_census_workspace_bytes(1, 10)) + 17 * 33 * 10 + int(L.rmem_label_edt_workspace_bytes(1, 17, 33))
    assert np.array_equal(surface.surface_census(da, db, 10, (1, 4), workspace_bytes=one).cpu().numpy(), want)          # one frame per pass
    assert np.array_equal(surface.surface_census(da, db, 10, (1, 4), workspace_bytes=2 * one + 1).cpu().numpy(), want)  # 2 + 1
    with pytest.raises(RmemError, match='workspace_bytes'):
        surface.surface_census(da, db, 10, workspace_bytes=one - 1)
    assert np.array_equal(surface.surface_census(da[0], db[0], 3, q=0).cpu().numpy(), R.census(a[0], b[0], 3, (), 0))
    big = (2, 37, 131)
    a, b = _pair(big)
    da, db = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs = [surface.surface_census(da, db, 10, (0, 1, 4, 2 ** 30 - 1), 5000) for _ in range(2)]
    side.synchronize()
    assert torch.equal(runs[0], runs[1]) and np.array_equal(runs[0].cpu().numpy(), R.census(a, b, 10, (0, 1, 4, 2 ** 30 - 1), 5000))


@pytest.mark.parametrize('pooled', [True, False], ids=['pooled', 'directed'])
def test_surface_metrics(dev, pooled):
    """hd and nsd exactly; hd95 within 1e-9 * max(1, value): double rounding is the only difference; assd within 2^-16 + 1e-9: the
    fixed point rounds every sample down by less than 2^-16"""
    from rmem_ocu_amd import evaluator, surface
    a, b = _pair((2, 37, 131))
    da, db = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    for tolerances, percentile in (((1.0, 2.0), 95.0), ((0.0, 1.5, 3.0, 30.0), 50.0), ((), 99.99)):
        want = R.metrics(a, b, 10, tolerances, percentile, pooled)
        got = surface.surface_metrics(da, db, 10, tolerances, percentile, pooled)
        assert set(got) == {'hd', 'hd95', 'assd', 'nsd'} and all(v.dtype == np.float64 for v in got.values())
        assert got['hd'].shape == (2, 10) and got['nsd'].shape == (2, 10, len(tolerances))
        assert np.array_equal(got['hd'], want['hd']) and np.array_equal(got['nsd'], want['nsd'])
        fin = np.isfinite(want['hd'])
        assert np.isinf(want['hd'][1, 1]) and (want['hd'][:, 6] == 0).all() and (want['nsd'][:, 6] == 1).all() and fin.sum() >= 14
        for k in ('hd95', 'assd'):
            assert np.array_equal(np.isfinite(got[k]), fin) and np.array_equal(got[k][~fin], want[k][~fin])
        assert (np.abs(got['hd95'][fin] - want['hd95'][fin]) <= 1e-9 * np.maximum(1.0, want['hd95'][fin])).all()
        assert (np.abs(got['assd'][fin] - want['assd'][fin]) <= 2.0 ** -16 + 1e-9).all()
        assert (got['assd'][fin] <= want['assd'][fin] + 1e-9).all()
    again = evaluator.surface_metrics(da, db, 10, pooled=pooled)
    first = surface.surface_metrics(da, db, 10, pooled=pooled)
    assert all(np.array_equal(again[k], first[k]) for k in first)
