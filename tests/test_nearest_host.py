"""The nearest-site transform's references against each other, against scipy and against frames written out by hand, the workspace
size, and every refusal the host makes before anything is launched (no GPU in this tier)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt

import nearest_ref as R
from conftest import ROOT

S = R.SENTINEL
LIMITS = (-1, 0, 1, 2, 4, 5, 50)
SETS = (({2}, None), ({0}, {2, 4}), ({2, 4}, {0}), ({0, 2, 4}, {0, 4}), ((), None), ({255}, {0}))      # (sites, fill)


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    return _lib.lib()


def _cases():
    rng = np.random.default_rng(23)
    for H in range(1, 10):
        for W in range(1, 13):
            nv = 1 + (H + W) % 3
            yield rng.integers(0, nv, (2, H, W)).astype(np.uint8) * 2          # values 0, 2, 4: value 2 is absent when nv == 1
            small = rng.integers(0, 3, (2, (H + 2) // 3, (W + 2) // 3)).astype(np.uint8)
            yield np.kron(small, np.ones((1, 3, 3), dtype=np.uint8))[:, :H, :W] * 2  # 3 x 3-blocky


def test_separable_equals_brute_force():
    """the two passes with "above wins a tie" give the lexicographic minimum of (d2, index) over all sites"""
    count = 0
    for k, a in enumerate(_cases()):
        for j in range(2):
            sites, fill = SETS[(k + 3 * j) % len(SETS)]
            want, got, few = R.brute_keys(a, sites), R.separable_keys(a, sites), R.separable_keys(a, sites, bound=True)
            assert np.array_equal(want, got) and np.array_equal(want, few), (a, sites)
            if a.size <= 24:
                assert np.array_equal(want, R.sparse_keys(a, sites))
            for max_d2 in LIMITS:
                w, g = R.finish(a, want, fill, max_d2), R.separable(a, sites, fill, max_d2)
                assert all(x.dtype == t and x.shape == a.shape for x, t in zip(w, (np.int32, np.int32, np.uint8)))
                assert all(np.array_equal(x, y) for x, y in zip(w, g)), (a, sites, fill, max_d2)
                index, dist2, taken = w
                assert ((index < 0) == (dist2 == S)).all() and (max_d2 < 0 or (dist2[index >= 0] <= max_d2).all())
                count += 1
    assert count == 9 * 12 * 2 * 2 * len(LIMITS)


def test_limits_and_fill_by_hand():
    a = np.array([[0, 0, 0, 7, 0],
                  [0, 5, 0, 0, 0],
                  [0, 0, 0, 0, 9]], dtype=np.uint8)
    for ref in (R.brute, R.separable, R.sparse):
        index, dist2, taken = ref(a, {5, 7}, {0}, -1)
        assert index.tolist() == [[6, 6, 3, 3, 3], [6, 6, 6, 3, 3], [6, 6, 6, 3, 3]]         # (1, 3): 7 at d2 1 beats 5 at d2 4
        assert dist2.tolist() == [[2, 1, 1, 0, 1], [1, 0, 1, 1, 2], [2, 1, 2, 4, 5]]
        assert taken.tolist() == [[5, 5, 7, 7, 7], [5, 5, 5, 7, 7], [5, 5, 5, 7, 9]]         # 9 is no site and not in fill: it stays
        index, dist2, taken = ref(a, {5, 7}, {0}, 1)                                         # d2 == max_d2 still counts
        assert index.tolist() == [[-1, 6, 3, 3, 3], [6, 6, 6, 3, -1], [-1, 6, -1, -1, -1]]
        assert dist2.tolist() == [[S, 1, 1, 0, 1], [1, 0, 1, 1, S], [S, 1, S, S, S]]
        assert taken.tolist() == [[0, 5, 7, 7, 7], [5, 5, 5, 7, 0], [0, 5, 0, 0, 9]]
        index, dist2, taken = ref(a, {5, 7}, {0}, 0)
        assert (index >= 0).sum() == 2 and np.array_equal(taken, a)
        index, dist2, taken = ref(a, (), None, -1)                                           # an empty site set is legal
        assert (index == -1).all() and (dist2 == S).all() and np.array_equal(taken, a)
        index, dist2, taken = ref(a, {0, 5}, {0, 9}, -1)                                     # fill pixels that are sites map to themselves
        assert taken.tolist() == [[0, 0, 0, 7, 0], [0, 5, 0, 0, 0], [0, 0, 0, 0, 0]]


def test_against_scipy():
    """dist2 is scipy's squared transform; the site scipy returns is ONE of the equally near ones, not always the first"""
    for k, a in enumerate(_cases()):
        if k % 4:
            continue
        for sites in ({2}, {0, 4}):
            index, dist2, _ = R.separable(a, sites)
            for f in range(a.shape[0]):
                site = np.isin(a[f], list(sites))
                if not site.any():
                    assert (index[f] == -1).all() and (dist2[f] == S).all()
                    continue
                d, (iy, ix) = distance_transform_edt(~site, return_indices=True)
                assert np.array_equal(np.rint(d ** 2).astype(np.int32), dist2[f])
                yy, xx = np.mgrid[0:a.shape[1], 0:a.shape[2]]
                assert site[iy, ix].all() and np.array_equal((iy - yy) ** 2 + (ix - xx) ** 2, dist2[f])
                assert (index[f] <= iy * a.shape[2] + ix).all()                              # ours is the first of them


def test_tie_frames_written_out_by_hand():
    for sites_at, pixel, want in R.TIES:
        a = R.tie_frame(sites_at)
        for ref in (R.brute, R.separable, R.sparse):
            index, dist2, taken = ref(a, {3}, {0})
            assert index[pixel] == want and taken[pixel] == 3, (sites_at, pixel, index)
            assert all(index[y, x] == 3 * y + x and dist2[y, x] == 0 for y, x in sites_at)   # a site maps to itself
    # the last pattern moved so that the same-row site lies in the next column segment of 32, and in the one before
    a = R.tie_frame(((1, 0), (0, 1)), (17, 70), (5, 31))[None]
    for ref in (R.brute, R.separable, R.sparse):
        assert ref(a, {3})[0][0, 5, 31] == 5 * 70 + 32
    b = np.zeros((1, 17, 70), dtype=np.uint8)
    b[0, 5, 31] = b[0, 6, 32] = 3
    for ref in (R.brute, R.separable, R.sparse):
        assert ref(b, {3})[0][0, 5, 32] == 5 * 70 + 31


def test_bits():
    assert R.bits({0, 3, 31, 32, 255}) == [1 | 8 | 1 << 31, 1, 0, 0, 0, 0, 0, 1 << 31]
    from rmem_ocu_amd import distance
    assert list(distance._bits({0, 3, 31, 32, 255})) == R.bits({0, 3, 31, 32, 255}) and list(distance._bits(())) == [0] * 8


def test_workspace_size(lib):
    assert lib.rmem_label_nearest_workspace_bytes(2, 3, 5) == 64     # 2 * 3 * 5 offsets of 16 bits = 60, in 16-byte units
    assert lib.rmem_label_nearest_workspace_bytes(1, 480, 854) == 480 * 854 * 2
    assert lib.rmem_label_nearest_workspace_bytes(1, 1, 16384) == 32768 and lib.rmem_label_nearest_workspace_bytes(1, 16384, 1) == 32768
    for n, H, W in ((0, 3, 5), (65536, 3, 5), (1, 0, 5), (1, 3, -1), (1, 16385, 1), (1, 1, 16385), (1, 16384, 16384)):
        assert lib.rmem_label_nearest_workspace_bytes(n, H, W) == 0, (n, H, W)


def test_c_entry_point_refuses_on_the_host(lib):
    """non-zero, a message that names the entry point, and nothing launched: the device pointers are never looked through"""
    P, Q, n, H, W = 4096, 8192, 2, 3, 5                              # non-null, aligned addresses
    need = lib.rmem_label_nearest_workspace_bytes(n, H, W)
    some = (ctypes.c_uint * 8)(8, 0, 0, 0, 0, 0, 0, 0)

    def run(labels=P, n=n, H=H, W=W, sites=some, fill=None, max_d2=-1, index=Q, dist2=Q, taken=Q, ws=P, ws_bytes=need):
        return lib.rmem_label_nearest(labels, n, H, W, sites, fill, max_d2, index, dist2, taken, ws, ws_bytes, None)

    for kw, msg in ((dict(labels=None), b'null pointer'), (dict(sites=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                    (dict(index=None, dist2=None, taken=None), b'no output'), (dict(taken=P), b'taken must not be labels'),
                    (dict(index=None, dist2=None, taken=P), b'taken must not be labels'),
                    (dict(n=0), b'n must be'), (dict(n=65536), b'n must be'), (dict(H=0), b'must be positive'), (dict(W=-1), b'must be positive'),
                    (dict(n=1, H=16385, W=1), b'at most 16384'), (dict(n=1, H=1, W=16385), b'at most 16384'),
                    (dict(n=1, H=16384, W=16384), b'at most 2^26'), (dict(max_d2=-2), b'max_d2 must be'),
                    (dict(max_d2=2 ** 30 + 1), b'max_d2 must be'), (dict(ws_bytes=need - 1), b'workspace too small'),
                    (dict(ws=P + 2), b'4-byte aligned')):
        assert run(**kw) != 0, kw
        err = lib.rmem_last_error_string()
        assert err.startswith(b'rmem_label_nearest:') and msg in err, (kw, err)


def test_python_functions_refuse_on_the_host():
    from rmem_ocu_amd import distance, evaluator
    from rmem_ocu_amd._lib import RmemError
    host = torch.zeros(2, 3, 5, dtype=torch.uint8)
    for fn in (lambda t: distance.nearest(t, {1}), distance.grow, lambda t: evaluator.expand_masks(t, 2), evaluator.fill_void,
               evaluator.labels_from_seeds):
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host)
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host.int())
    for bad in (3, 'abc', [256], [-1], [1.5], [True], torch.zeros(2)):
        with pytest.raises(RmemError, match='sites must be an iterable of integers in 0..255'):
            distance.nearest(host, bad)
        with pytest.raises(RmemError, match='fill must be an iterable of integers in 0..255'):
            distance.grow(host, fill=bad)
    with pytest.raises(RmemError, match='sites must be an iterable of integers in 0..255'):
        distance.grow(host, sites=[300])
    for fn in (lambda **kw: distance.nearest(host, {1}, **kw), lambda **kw: distance.grow(host, **kw)):
        with pytest.raises(RmemError, match='max_distance or max_d2, not both'):
            fn(max_distance=2, max_d2=4)
        for bad in (-1, 2 ** 30 + 1, 1.5, True):
            with pytest.raises(RmemError, match='max_d2 must be None or an integer in 0..1073741824'):
                fn(max_d2=bad)
        for bad in (-1, float('nan'), float('inf'), 'x', True):
            with pytest.raises(RmemError, match='max_distance must be None or a finite number'):
                fn(max_distance=bad)
    assert distance._limit('x', None, None) == -1 and distance._limit('x', 2, None) == 4 and distance._limit('x', 1.5, None) == 2
    assert distance._limit('x', None, 0) == 0 and distance._limit('x', 1e9, None) == 2 ** 30 and distance._limit('x', 0, None) == 0
    with pytest.raises(RmemError, match='distance must be a finite number'):
        evaluator.expand_masks(host, None)
    with pytest.raises(RmemError, match='max_distance must be None or a finite number'):
        evaluator.expand_masks(host, -1)
    for bad in (0, 256, 1.5):
        with pytest.raises(RmemError, match='void must be None or an integer in 1..255'):
            evaluator.expand_masks(host, 2, void=bad)
        with pytest.raises(RmemError, match='background must be None or an integer in 1..255'):
            evaluator.labels_from_seeds(host, background=bad)
    with pytest.raises(RmemError, match='void must be an integer in 0..255'):
        evaluator.fill_void(host, void=256)


def test_symbols_declared_exported_and_bound(lib):
    from rmem_ocu_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rmem.h')).read()
    assert re.search(r'#define\s+RMEM_ABI_VERSION\s+15\b', header) and lib.rmem_abi_version() == 15
    for name in ('rmem_label_nearest_workspace_bytes', 'rmem_label_nearest'):
        assert re.search(r'\b%s\s*\(' % name, header) and hasattr(lib, name) and name in _lib.SIGNATURES
        assert name not in _lib.F16_TWINS                            # uint8 in, integers out: built once
    assert len(_lib.SIGNATURES['rmem_label_nearest'][1]) == 13
    makefile = open(os.path.join(ROOT, 'rmem_ocu_amd', 'csrc', 'Makefile')).read()
    assert 'label_nearest.o' in makefile.split('OBJS')[1].split('\n')[0]
