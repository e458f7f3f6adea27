"""The geodesic nearest-site transform's two references against each other, against scipy's Dijkstra (the cost alone) and against
frames written out by hand, the workspace size, and every refusal the host makes before anything is launched (no GPU in this
tier)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import geodesic_ref as R
from conftest import ROOT

S = R.SENTINEL
WEIGHTS = ((1, 0), (1, 1), (64, 64), (5, 2))
SHAPES = ((1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 5, 6), (1, 13, 21))


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    return _lib.lib()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_jacobi_equals_dijkstra_on_every_generator():
    """with and without a limit; the limit is also the threshold of the unlimited keys (a prefix of a cheapest path is no dearer)"""
    count = 0
    for si, shape in enumerate(SHAPES):
        for ii, kind in enumerate(R.IMAGES):
            for C in (1, 3):
                image = R.make_image(kind, shape, C, tw=3)
                for li, lk in enumerate(R.LABELS):
                    labels = R.make_labels(lk, shape)
                    sites = R.SITE_SETS[(si + ii + li + C) % 5]
                    sp, co = WEIGHTS[(ii + li) % 4]
                    kj, kd = R.jacobi(labels, image, sites, sp, co), R.dijkstra(labels, image, sites, sp, co)
                    assert np.array_equal(kj, kd), (shape, kind, C, lk, sites)
                    cost = kj >> R.SHIFT
                    real = cost[cost != S]
                    for limit in (0, int(np.median(real)) if real.size else 7, 2 ** 30):
                        lj, ld = R.jacobi(labels, image, sites, sp, co, limit), R.dijkstra(labels, image, sites, sp, co, limit)
                        assert np.array_equal(lj, ld)
                        assert _same(R.finish(labels, lj, None, limit), R.finish(labels, kj, None, limit))
                        count += 1
    assert count == len(SHAPES) * len(R.IMAGES) * 2 * 3 * 3
    labels, image = R.serpentine((1, 12, 19))
    kj = R.jacobi(labels, image, (3,), 1, 64)
    assert np.array_equal(kj, R.dijkstra(labels, image, (3,), 1, 64))
    assert (kj >> R.SHIFT)[0, 0, 18] > 2 * 5 * 11 and ((kj & R.MASK) == 0).all()     # round two walls: down and up again


def test_cost_against_scipy():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    shape = (1, 9, 14)
    for kind, C, (sp, co) in (('random', 3, (1, 1)), ('wall', 1, (5, 2)), ('step', 3, (64, 64))):
        image, labels = R.make_image(kind, shape, C, tw=5), R.make_labels('sparse', shape)
        _, im = R.channels(labels, image)
        H, W = shape[1:]
        rows, cols, vals = [], [], []
        for y in range(H):
            for x in range(W):
                for dy, dx, s in R.STEPS:
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        rows.append(y * W + x)
                        cols.append((y + dy) * W + x + dx)
                        vals.append(sp * s + co * int(np.abs(im[0, y, x] - im[0, y + dy, x + dx]).sum()))
        g = coo_matrix((vals, (rows, cols)), shape=(H * W, H * W)).tocsr()
        sites = np.nonzero(np.isin(labels.reshape(-1), (1, 2, 3)))[0]
        d = dijkstra(g, indices=sites, min_only=True)
        assert np.array_equal(d.astype(np.int64).reshape(shape), R.jacobi(labels, image, (1, 2, 3), sp, co) >> R.SHIFT)


def test_frames_written_out_by_hand():
    # two sites symmetric about a pixel on a uniform image: the smaller flat index wins
    labels = np.zeros((3, 7), dtype=np.uint8)
    labels[1, 1] = labels[1, 5] = 3
    image = np.full((3, 7), 77, dtype=np.uint8)
    for ref in (R.jacobi, R.dijkstra):
        index, cost, taken = R.finish(labels, ref(labels, image, (3,)), (0,))
        assert index.tolist() == [[8, 8, 8, 8, 12, 12, 12]] * 3 and index[1, 3] == 8 and cost[1, 3] == 10
        assert cost.tolist() == [[7, 5, 7, 12, 7, 5, 7], [5, 0, 5, 10, 5, 0, 5], [7, 5, 7, 12, 7, 5, 7]] and (taken == 3).all()
    labels = np.zeros((5, 5), dtype=np.uint8)                        # the same across rows: the site above comes first
    labels[0, 2] = labels[4, 2] = 3
    for ref in (R.jacobi, R.dijkstra):
        assert R.finish(labels, ref(labels, np.zeros((5, 5), np.uint8), (3,)))[0][2].tolist() == [2] * 5
    # a one-pixel-wide bright wall with a gap: the path goes through the gap
    image = np.zeros((5, 5), dtype=np.uint8)
    image[:, 2] = 255
    image[4, 2] = 0
    labels = np.zeros((5, 5), dtype=np.uint8)
    labels[0, 0] = 1
    for ref in (R.jacobi, R.dijkstra):
        index, cost, _ = R.finish(labels, ref(labels, image, (1,), 1, 1))
        assert (index == 0).all()
        assert cost[4, 2] == 5 + 5 + 7 + 7                            # (0,0) (1,0) (2,0) (3,1) and into the gap (4,2)
        assert cost[0, 4] == 24 + 7 + 7 + 5 + 5                       # on through (3,3) (2,4) (1,4): twice the chamfer to the gap
        assert cost[0, 2] == 5 + 5 + 255                              # onto the wall itself: one step of |255 - 0| from (0,1)
        assert cost[0, 4] < 4 * 5 + 2 * 255                           # the straight way across the wall is dearer
    # colour = 0 against the chamfer by hand
    labels = np.zeros((9, 14), dtype=np.uint8)
    labels[6, 3] = 2
    image = R.make_image('random', (1, 9, 14), 3, 4)[0]
    for ref in (R.jacobi, R.dijkstra):
        for sp in (1, 5, 64):
            index, cost, _ = R.finish(labels, ref(labels, image, (2,), sp, 0))
            assert np.array_equal(cost, sp * R.chamfer(9, 14, 6, 3)) and (index == 6 * 14 + 3).all()


def test_limit_at_a_pixels_cost():
    labels, image = R.make_labels('sparse', (1, 13, 21)), R.make_image('random', (1, 13, 21), 1, 4)
    keys = R.jacobi(labels, image, (1, 2, 3))
    cost = keys >> R.SHIFT
    c = int(cost[0, 6, 10])
    assert 0 < c < S
    for ref in (R.jacobi, R.dijkstra):
        index, got, _ = R.finish(labels, ref(labels, image, (1, 2, 3), 1, 1, c), None, c)
        assert index[0, 6, 10] >= 0 and got[0, 6, 10] == c and (got[index >= 0] <= c).all()      # a cost == max_cost still counts
        index, got, _ = R.finish(labels, ref(labels, image, (1, 2, 3), 1, 1, c - 1), None, c - 1)
        assert index[0, 6, 10] == -1 and got[0, 6, 10] == S                                      # one less drops it
    index, got, taken = R.finish(labels, keys, (0,), 0)
    assert np.array_equal(index >= 0, np.isin(labels, (1, 2, 3))) and np.array_equal(taken, labels)
    index, got, taken = R.finish(labels, R.jacobi(labels, image, ()), None)                      # an empty site set is legal
    assert (index == -1).all() and (got == S).all() and np.array_equal(taken, labels)


def test_workspace_size(lib):
    th, tw = ctypes.c_int(), ctypes.c_int()
    assert lib.rmem_label_geodesic_tile(ctypes.byref(th), ctypes.byref(tw)) == 0 and (th.value, tw.value) == (32, 64)
    assert lib.rmem_label_geodesic_tile(None, ctypes.byref(tw)) != 0 and b'null pointer' in lib.rmem_last_error_string()
    # two planes of 8 bytes per pixel, two sets of one byte per tile, each rounded up to 16
    assert lib.rmem_label_geodesic_workspace_bytes(2, 3, 5) == 2 * 240 + 2 * 16
    assert lib.rmem_label_geodesic_workspace_bytes(1, 480, 854) == 2 * 480 * 854 * 8 + 2 * 224     # 15 x 14 = 210 tiles -> 224
    assert lib.rmem_label_geodesic_workspace_bytes(3, 33, 65) == 2 * 51488 + 2 * 16                # 3 * 33 * 65 * 8 = 51480, 12 tiles
    assert lib.rmem_label_geodesic_workspace_bytes(1, 1, 16384) == 2 * 131072 + 2 * 256
    for n, H, W in ((0, 3, 5), (65536, 3, 5), (1, 0, 5), (1, 3, -1), (1, 16385, 1), (1, 1, 16385), (1, 16384, 16384)):
        assert lib.rmem_label_geodesic_workspace_bytes(n, H, W) == 0, (n, H, W)


def test_c_entry_points_refuse_on_the_host(lib):
    """non-zero, a message that names the entry point, and nothing launched: the device pointers are never looked through"""
    P, Q, n, H, W = 4096, 8192, 2, 3, 5
    need = lib.rmem_label_geodesic_workspace_bytes(n, H, W)
    some = (ctypes.c_uint * 8)(8, 0, 0, 0, 0, 0, 0, 0)
    geometry = ((dict(n=0), b'n must be'), (dict(n=65536), b'n must be'), (dict(H=0), b'must be positive'), (dict(W=-1), b'must be positive'),
                (dict(n=1, H=16385, W=1), b'at most 16384'), (dict(n=1, H=1, W=16385), b'at most 16384'),
                (dict(n=1, H=16384, W=16384), b'at most 2^26'), (dict(ws=None), b'null pointer'),
                (dict(ws_bytes=need - 1), b'workspace too small'), (dict(ws=P + 8), b'16-byte aligned'))

    def begin(labels=P, n=n, H=H, W=W, sites=some, ws=P, ws_bytes=need):
        return lib.rmem_label_geodesic_begin(labels, n, H, W, sites, ws, ws_bytes, None)

    def rounds(image=P, C=3, n=n, H=H, W=W, spatial=1, colour=1, max_cost=-1, first=0, count=1, changed=Q, ws=P, ws_bytes=need):
        return lib.rmem_label_geodesic_rounds(image, C, n, H, W, spatial, colour, max_cost, first, count, changed, ws, ws_bytes, None)

    def finish(labels=P, n=n, H=H, W=W, fill=None, max_cost=-1, done=1, index=Q, cost=Q, taken=Q, ws=P, ws_bytes=need):
        return lib.rmem_label_geodesic_finish(labels, n, H, W, fill, max_cost, done, index, cost, taken, ws, ws_bytes, None)

    limits = ((dict(max_cost=-2), b'max_cost must be'), (dict(max_cost=2 ** 30 + 1), b'max_cost must be'))
    cases = {
        'begin': (begin, ((dict(labels=None), b'null pointer'), (dict(sites=None), b'null pointer')) + geometry),
        'rounds': (rounds, ((dict(image=None), b'null pointer'), (dict(changed=None), b'null pointer'), (dict(C=0), b'channels must be 1 or 3'),
                            (dict(C=2), b'channels must be 1 or 3'), (dict(C=4), b'channels must be 1 or 3'),
                            (dict(spatial=0), b'spatial must be'), (dict(spatial=65), b'spatial must be'), (dict(colour=-1), b'colour must be'),
                            (dict(colour=65), b'colour must be'), (dict(first=-1), b'first_round must not be negative'),
                            (dict(count=0), b'count must be at least 1'), (dict(count=-3), b'count must be at least 1'),
                            (dict(first=2 ** 31 - 4, count=4), b'must fit 31 bits')) + limits + geometry),
        'finish': (finish, ((dict(labels=None), b'null pointer'), (dict(index=None, cost=None, taken=None), b'no output'),
                            (dict(taken=P), b'taken must not be labels'), (dict(index=None, cost=None, taken=P), b'taken must not be labels'),
                            (dict(done=-1), b'rounds must not be negative')) + limits + geometry),
    }
    for name, (fn, refusals) in cases.items():
        for kw, msg in refusals:
            assert fn(**kw) != 0, (name, kw)
            err = lib.rmem_last_error_string()
            assert err.startswith(b'rmem_label_geodesic_%s:' % name.encode()) and msg in err, (name, kw, err)


def test_python_functions_refuse_on_the_host():
    from rmem_ocu_amd import distance, evaluator
    from rmem_ocu_amd._lib import RmemError
    host, image = torch.zeros(2, 3, 5, dtype=torch.uint8), torch.zeros(2, 3, 5, 3, dtype=torch.uint8)
    fns = (lambda t, i, **kw: distance.geodesic_nearest(t, i, {1}, **kw), distance.geodesic_grow, evaluator.labels_from_seeds_geodesic,
           evaluator.fill_void_geodesic)
    for fn in fns + (lambda t, i: evaluator.snap_masks(t, i, 3),):
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host, image)
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host.int(), image)
    for bad in (3, 'abc', [256], [-1], [1.5], [True], torch.zeros(2)):
        with pytest.raises(RmemError, match='sites must be an iterable of integers in 0..255'):
            distance.geodesic_nearest(host, image, bad)
        with pytest.raises(RmemError, match='fill must be an iterable of integers in 0..255'):
            distance.geodesic_grow(host, image, fill=bad)
    with pytest.raises(RmemError, match='sites must be an iterable of integers in 0..255'):
        distance.geodesic_grow(host, image, sites=[300])
    for fn in fns:
        for bad in (0, 65, 1.5, True, None):
            with pytest.raises(RmemError, match='spatial must be an integer in 1..64'):
                fn(host, image, spatial=bad)
        for bad in (-1, 65, 0.5, True, None):
            with pytest.raises(RmemError, match='colour must be an integer in 0..64'):
                fn(host, image, colour=bad)
        for bad in (-1, 2 ** 30 + 1, 1.5, True):
            with pytest.raises(RmemError, match='max_cost must be None or an integer in 0..1073741824'):
                fn(host, image, max_cost=bad)
    for fn in fns[:2]:
        for bad in (0, -1, 2 ** 20 + 1, 2.0, True):
            with pytest.raises(RmemError, match='batch must be an integer in 1..1048576'):
                fn(host, image, batch=bad)
    for bad in (0, 256, 1.5):
        with pytest.raises(RmemError, match='background must be None or an integer in 1..255'):
            evaluator.labels_from_seeds_geodesic(host, image, background=bad)
    with pytest.raises(RmemError, match='void must be an integer in 0..255'):
        evaluator.fill_void_geodesic(host, image, void=256)
    for bad in (0, 0.5, 64, True, None, 'x'):
        with pytest.raises(RmemError, match='band must be a number in 1..63'):
            evaluator.snap_masks(host, image, bad)
    with pytest.raises(RmemError, match='unknown must be an integer in 0..255'):
        evaluator.snap_masks(host, image, 3, unknown=-1)
    # the image against the labels: every failure has a message of its own (the labels here stand for a device stack)
    labels = torch.zeros(2, 3, 5, dtype=torch.uint8, device='meta')
    a = labels
    for bad, msg in ((None, 'image must be a uint8 tensor'), (torch.zeros(2, 3, 5, 3, device='meta'), 'image must be a uint8 tensor'),
                     (image, 'image must be on the labels\' device'),
                     (torch.zeros(2, 3, 5, 2, dtype=torch.uint8, device='meta'), 'image must have the labels\' shape'),
                     (torch.zeros(2, 3, 6, dtype=torch.uint8, device='meta'), 'image must have the labels\' shape'),
                     (torch.zeros(3, 5, 3, dtype=torch.uint8, device='meta'), 'image must have the labels\' shape'),
                     (torch.zeros(2, 3, 3, 5, dtype=torch.uint8, device='meta').permute(0, 1, 3, 2), 'image must be contiguous')):
        with pytest.raises(RmemError, match=msg):
            distance._image('x', bad, labels, a)
    for shape, C in (((2, 3, 5), 1), ((2, 3, 5, 1), 1), ((2, 3, 5, 3), 3)):
        img, got = distance._image('x', torch.zeros(shape, dtype=torch.uint8, device='meta'), labels, a)
        assert got == C and img.shape == (2, 3, 5, C)
    img, got = distance._image('x', torch.zeros(3, 5, 3, dtype=torch.uint8, device='meta'), labels[0], labels[:1])
    assert got == 3 and img.shape == (1, 3, 5, 3)
    assert distance._cost_limit('x', None) == -1 and distance._cost_limit('x', 0) == 0 and distance._cost_limit('x', 2 ** 30) == 2 ** 30


def test_symbols_declared_exported_and_bound(lib):
    from rmem_ocu_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rmem.h')).read()
    assert re.search(r'#define\s+RMEM_ABI_VERSION\s+15\b', header) and lib.rmem_abi_version() == 15
    names = ('rmem_label_geodesic_tile', 'rmem_label_geodesic_workspace_bytes', 'rmem_label_geodesic_begin', 'rmem_label_geodesic_rounds',
             'rmem_label_geodesic_finish')
    for name in names:
        assert re.search(r'\b%s\s*\(' % name, header) and hasattr(lib, name) and name in _lib.SIGNATURES
        assert name not in _lib.F16_TWINS                            # uint8 in, integers out: built once
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [2, 3, 8, 14, 13]
    makefile = open(os.path.join(ROOT, 'rmem_ocu_amd', 'csrc', 'Makefile')).read()
    assert 'label_geodesic.o' in makefile.split('OBJS')[1].split('\n')[0]
    assert re.search(r'label_geodesic\.o[^\n]*: label_scan\.h label_wave\.h', makefile)
    from rmem_ocu_amd import distance, evaluator
    assert all(callable(getattr(distance, f)) for f in ('geodesic_nearest', 'geodesic_grow', 'geodesic_tile'))
    assert all(callable(getattr(evaluator, f)) for f in ('labels_from_seeds_geodesic', 'fill_void_geodesic', 'snap_masks'))
