"""The surface metrics' references against each other and against a hand-written frame, the census rows at their edges, the rank
formula against numpy, the workspace sizes, and every refusal the host makes before anything is launched (no GPU in this tier)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import surface_ref as R

S = R.SENTINEL
HAND_A = np.array([[0, 0, 0, 0, 0],
                   [0, 1, 1, 1, 0],
                   [0, 1, 1, 1, 0],
                   [0, 1, 1, 1, 0]], dtype=np.uint8)
HAND_B = np.array([[0, 0, 0, 0, 0],
                   [0, 1, 0, 0, 0],
                   [0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0]], dtype=np.uint8)


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    return _lib.lib()


def _cases():
    rng = np.random.default_rng(22)
    for H in range(1, 10):
        for W in range(1, 13):
            nv = 1 + (H + W) % 3
            yield rng.integers(0, nv, (2, H, W)).astype(np.uint8)
            small = rng.integers(0, 3, (2, (H + 2) // 3, (W + 2) // 3)).astype(np.uint8)
            yield np.kron(small, np.ones((1, 3, 3), dtype=np.uint8))[:, :H, :W]  # 3 x 3-blocky


def test_the_two_surfaces_and_the_two_sample_routes_agree():
    count = 0
    for a in _cases():
        s = R.surface(a)
        assert s.dtype == np.uint8 and s.shape == a.shape and np.array_equal(s, R.surface_erosion(a)), a
        assert ((s == a) | (s == 0)).all() and (s[a == 0] == 0).all()
        b = np.ascontiguousarray(a[::-1])                            # the other frame of the pair
        want, got = R.samples(a, b, 2), R.samples_edt(a, b, 2)
        assert all(np.array_equal(w, g) for w, g in zip(want, got)), a
        count += 1
    assert count == 9 * 12 * 2 >= 200


def test_a_frame_written_out_by_hand():
    assert R.surface(HAND_A).tolist() == [[0, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 0, 1, 0], [0, 1, 1, 1, 0]]     # the last row touches the edge
    assert np.array_equal(R.surface(HAND_B), HAND_B) and np.array_equal(R.surface_erosion(HAND_A), R.surface(HAND_A))
    for route in (R.samples, R.samples_edt):
        da, db = route(HAND_A, HAND_B, 1)
        assert da.tolist() == [[-1, -1, -1, -1, -1], [-1, 0, 1, 4, -1], [-1, 1, -1, 5, -1], [-1, 4, 5, 8, -1]]
        assert db.tolist() == [[-1] * 5, [-1, 0, -1, -1, -1], [-1] * 5, [-1] * 5]
    # a -> b: 0 1 1 4 4 5 5 8, ranks 6 and 7 of 8 (7 * 9500 = 66500); roots in 2^-16: 0, 65536, 131072, 146542 (sqrt 5), 185363 (sqrt 8)
    fix = 2 * 65536 + 2 * 131072 + 2 * 146542 + 185363
    assert fix == 871663 == sum(math.isqrt(v << 32) for v in (0, 1, 1, 4, 4, 5, 5, 8))
    table = R.census(HAND_A, HAND_B, 1, tol2=(1, 4), q=9500)
    assert table.shape == (1, 1, 3, 9)
    assert table[0, 0].tolist() == [[8, fix, 8, 5, 8, 3, 5, 0, 0],
                                    [1, 0, 0, 0, 0, 1, 1, 0, 0],
                                    [9, fix, 8, 5, 8, 4, 6, 0, 0]]   # pooled: 0 0 1 1 4 4 5 5 8, ranks 7 and 8 (8 * 9500 = 76000)
    assert np.array_equal(table, R.census(HAND_A, HAND_B, 1, (1, 4), 9500, R.samples(HAND_A, HAND_B, 1)))
    m = R.metrics(HAND_A, HAND_B, 1, tolerances=(1.0, 2.0))
    assert m['hd'][0, 0] == math.sqrt(8) and m['nsd'][0, 0].tolist() == [4 / 9, 6 / 9]
    assert abs(m['hd95'][0, 0] - (math.sqrt(5) + 0.6 * (math.sqrt(8) - math.sqrt(5)))) < 1e-12
    assert abs(m['assd'][0, 0] - fix / 9 / 65536) < 2.0 ** -16


def test_census_rows_at_their_edges():
    assert R.census_row([]) == (0, 0, -1, -1, -1, 0, 0, 0, 0)
    assert R.census_row([S, S, S], (0, 2 ** 30 - 1)) == (3, 0, S, S, S, 0, 0, 0, 0)
    assert R.census_row([7], (6, 7), q=0) == R.census_row([7], (6, 7), q=10000) == (1, math.isqrt(7 << 32), 7, 7, 7, 0, 1, 0, 0)
    assert R.census_row([9, 4], q=0)[2:5] == (9, 4, 9)               # m = 2: rank 0, then 1
    assert R.census_row([9, 4], q=9999)[2:5] == (9, 4, 9) and R.census_row([9, 4], q=10000)[2:5] == (9, 9, 9)
    assert R.census_row([9, 4], (4, 8, 9, 3))[5:] == (1, 1, 2, 0)
    empty = np.zeros((1, 3, 4), dtype=np.uint8)
    one = empty.copy()
    one[0, 1, 1:3] = 1
    t = R.census(one, empty, 2)                                      # object 1 on one side only, object 2 on neither
    assert t[0, 0].tolist() == [[2, 0, S, S, S, 0, 0, 0, 0], list(R.EMPTY_ROW), [2, 0, S, S, S, 0, 0, 0, 0]]
    assert t[0, 1].tolist() == [list(R.EMPTY_ROW)] * 3
    m = R.metrics(one, empty, 2)
    assert np.isinf(m['hd'][0, 0]) and np.isinf(m['hd95'][0, 0]) and np.isinf(m['assd'][0, 0]) and (m['nsd'][0, 0] == 0).all()
    assert m['hd'][0, 1] == 0 and m['assd'][0, 1] == 0 and (m['nsd'][0, 1] == 1).all()


def test_rank_formula_is_numpys_linear_percentile():
    rng = np.random.default_rng(23)
    for m in (1, 2, 3, 7, 100, 1001):
        d2 = np.sort(rng.integers(0, 5000, m))
        for q in (0, 1, 5000, 9500, 9999, 10000):
            row = R.census_row(d2, q=q)
            frac = ((m - 1) * q % 10000) / 10000
            got = math.sqrt(row[3]) + frac * (math.sqrt(row[4]) - math.sqrt(row[3]))
            want = float(np.percentile(np.sqrt(d2.astype(np.float64)), q / 100))
            assert abs(got - want) <= 1e-9 * max(1.0, want), (m, q, got, want)


def test_metrics_from_table_equals_the_float_reference():
    """the host half of surface_metrics, fed with the reference's table"""
    from rmem_ocu_amd.surface import metrics_from_table
    rng = np.random.default_rng(24)
    a = np.kron(rng.integers(0, 4, (3, 4, 5)).astype(np.uint8), np.ones((1, 3, 3), dtype=np.uint8))
    b = np.roll(a, (1, 2), axis=(1, 2))
    b[1][b[1] == 2] = 0                                              # object 2 absent on one side of frame 1; object 4 on both, everywhere
    for pooled in (True, False):
        want = R.metrics(a, b, 4, (1.0, 2.5), 95.0, pooled)
        got = metrics_from_table(R.census(a, b, 4, (1, 6), 9500), 9500, 2, pooled)
        assert np.isinf(want['hd'][1, 1]) and (want['nsd'][:, 3] == 1).all()
        assert np.array_equal(got['hd'], want['hd']) and np.array_equal(got['nsd'], want['nsd'])
        fin = np.isfinite(want['hd95'])
        assert np.array_equal(fin, np.isfinite(got['hd95'])) and np.array_equal(fin, np.isfinite(got['assd']))
        assert (np.abs(got['hd95'][fin] - want['hd95'][fin]) <= 1e-9 * np.maximum(1.0, want['hd95'][fin])).all()
        assert (np.abs(got['assd'][fin] - want['assd'][fin]) <= 2.0 ** -16 + 1e-9).all()


def test_workspace_sizes(lib):
    per_object = 2 * 7 * 8 + 3 * 8 * 4 + 3 * 1024 * 4                # two directed rows of 7 int64, three states of 8 int32, three histograms
    assert per_object == 12496
    assert lib.rmem_surface_census_workspace_bytes(2, 3) == 6 * per_object
    assert lib.rmem_surface_census_workspace_bytes(65535, 255) == 65535 * 255 * per_object
    for n, k in ((0, 3), (65536, 3), (1, 0), (1, 256), (-1, -1)):
        assert lib.rmem_surface_census_workspace_bytes(n, k) == 0, (n, k)


def test_c_entry_points_refuse_on_the_host(lib):
    """non-zero, a message, and nothing launched: the pointers are never looked through"""
    P, n, H, W = 4096, 2, 3, 5                                       # a non-null, aligned address

    def check(fn, cases):
        for kw, msg in cases:
            assert fn(**kw) != 0, kw
            assert msg in lib.rmem_last_error_string(), (kw, lib.rmem_last_error_string())

    def surface(labels=P, n=n, H=H, W=W, out=P):
        return lib.rmem_label_surface(labels, n, H, W, out, None)

    geometry = [(dict(n=0), b'n must be'), (dict(n=65536), b'n must be'), (dict(H=0), b'must be positive'), (dict(W=-1), b'must be positive'),
                (dict(n=1, H=16384, W=16384), b'at most 2^26'), (dict(n=1, H=16385, W=1), b'at most 16384'),
                (dict(n=1, H=1, W=16385), b'at most 16384')]
    check(surface, [(dict(labels=None), b'null pointer'), (dict(out=None), b'null pointer')] + geometry)
    assert b'rmem_label_surface' in lib.rmem_last_error_string()
    need = lib.rmem_label_edt_workspace_bytes(n, H, W)

    def at(labels=P, keys=P, n=n, H=H, W=W, value=1, key=1, samples=P, ws=P, ws_bytes=need):
        return lib.rmem_label_edt_at(labels, keys, n, H, W, value, key, samples, ws, ws_bytes, None)

    check(at, [(dict(labels=None), b'null pointer'), (dict(keys=None), b'null pointer'), (dict(samples=None), b'null pointer'),
               (dict(ws=None), b'null pointer')] + geometry +
          [(dict(value=-1), b'value must be in 0..255'), (dict(value=256), b'value must be in 0..255'), (dict(key=-1), b'key must be in 0..255'),
           (dict(key=256), b'key must be in 0..255'), (dict(ws_bytes=need - 1), b'workspace too small'), (dict(ws=P + 2), b'4-byte aligned')])
    assert b'rmem_label_edt_at' in lib.rmem_last_error_string()
    cneed = lib.rmem_surface_census_workspace_bytes(n, 3)
    tol = (ctypes.c_int * 4)(0, 1, 4, 2 ** 30 - 1)

    def census(sa=P, ka=P, sb=P, kb=P, n=n, H=H, W=W, num_objs=3, tol2=tol, num_tol=4, q=9500, table=P, ws=P, ws_bytes=cneed):
        return lib.rmem_surface_census(sa, ka, sb, kb, n, H, W, num_objs, tol2, num_tol, q, table, ws, ws_bytes, None)

    check(census, [(dict(sa=None), b'null pointer'), (dict(ka=None), b'null pointer'), (dict(sb=None), b'null pointer'),
                   (dict(kb=None), b'null pointer'), (dict(table=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                   (dict(tol2=None), b'tol2 is required')] + geometry +
          [(dict(num_objs=0), b'num_objs must be in 1..255'), (dict(num_objs=256), b'num_objs must be in 1..255'),
           (dict(num_tol=-1), b'num_tol must be in 0..4'), (dict(num_tol=5), b'num_tol must be in 0..4'), (dict(q=-1), b'q must be in 0..10000'),
           (dict(q=10001), b'q must be in 0..10000'), (dict(tol2=(ctypes.c_int * 4)(0, 1, -1, 0)), b'every tol2 must be'),
           (dict(tol2=(ctypes.c_int * 4)(0, 1, 2, 2 ** 30)), b'every tol2 must be'), (dict(ws_bytes=cneed - 1), b'workspace too small'),
           (dict(ws=P + 4), b'8-byte aligned')])
    assert b'rmem_surface_census' in lib.rmem_last_error_string()


def test_python_functions_refuse_on_the_host():
    from rmem_ocu_amd import evaluator, surface
    from rmem_ocu_amd._lib import RmemError
    host = torch.zeros(2, 3, 5, dtype=torch.uint8)
    samples = torch.zeros(2, 3, 5, dtype=torch.int32)
    for bad in (host, host.int()):
        with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
            surface.label_surface(bad)
        with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
            surface.edt_at(bad, bad, 1, 1, samples)
    for value, key, name in ((256, 1, 'value'), (-1, 1, 'value'), (1, 256, 'key'), (1, 1.5, 'key'), (True, 1, 'value')):
        with pytest.raises(RmemError, match=f'{name} must be an integer in 0..255'):
            surface.edt_at(host, host, value, key, samples)
    for fn in (surface.surface_census, surface.surface_metrics, evaluator.surface_metrics):
        for bad in (0, 256, 1.5, True):
            with pytest.raises(RmemError, match='num_objs must be an integer in 1..255'):
                fn(host, host, bad)
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host, host, 3)
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host.float(), host.float(), 3)
    for bad in ((1, 2, 3, 4, 5), 3, (1.5,), (-1,), (2 ** 30,)):
        with pytest.raises(RmemError, match='tol2 must be'):
            surface.surface_census(host, host, 3, tol2=bad)
    for bad in (-1, 10001, 95.0, True):
        with pytest.raises(RmemError, match='q must be an integer in 0..10000'):
            surface.surface_census(host, host, 3, q=bad)
    for fn in (surface.surface_metrics, evaluator.surface_metrics):
        for bad in ((1, 2, 3, 4, 5), 2.0, (-1.0,), (40000.0,), ('1',)):
            with pytest.raises(RmemError, match='tolerance'):
                fn(host, host, 3, tolerances=bad)
        for bad in (-1, 100.5, 95.001, '95', True):
            with pytest.raises(RmemError, match='percentile must be'):
                fn(host, host, 3, percentile=bad)


def test_new_symbols_are_declared_exported_and_bound(lib):
    """what tests/test_abi.py checks for every symbol, spelled out for the four new ones; the ABI version stays"""
    import test_abi
    from rmem_ocu_amd import _lib
    names = test_abi.declared_symbols()
    for name in ('rmem_label_surface', 'rmem_label_edt_at', 'rmem_surface_census_workspace_bytes', 'rmem_surface_census'):
        assert name in names and hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rmem_abi_version() == _lib.ABI_VERSION == 15
