"""The pair census without a GPU: the numpy restatement (pair_ref.census) against tables written out by hand, pairs.pair_iou /
track_iou from tables against the definitions on boolean masks, pairs.assign against brute force (and scipy where it imports),
and every refusal of the C entry point and of the Python functions."""
import os

import numpy as np
import pytest

import pair_ref


# ------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_against_tables_by_hand():
    a = np.array([[[0, 1, 1], [2, 2, 0]]], dtype=np.uint8)          # a 2 x 3 frame
    b = np.array([[[0, 1, 2], [2, 2, 1]]], dtype=np.uint8)
    assert pair_ref.census(a, b, 2, 2).tolist() == [[[1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 2, 0], [0, 0, 0, 0]]]
    a = np.array([[[1, 1, 0], [0, 1, 0]]], dtype=np.uint8)          # void in b: the last column
    b = np.array([[[1, 255, 255], [0, 0, 1]]], dtype=np.uint8)
    assert pair_ref.census(a, b, 1, 1).tolist() == [[[1, 1, 1], [1, 1, 1], [0, 0, 0]]]
    a = np.array([[[5, 1, 0], [2, 200, 1]]], dtype=np.uint8)        # values above num_a: the last row; b's 3 above num_b = 2
    b = np.array([[[1, 1, 0], [2, 2, 3]]], dtype=np.uint8)
    assert pair_ref.census(a, b, 1, 2).tolist() == [[[1, 0, 0, 0], [0, 1, 0, 1], [0, 1, 2, 0]]]


def _stacks(seed=5, shape=(3, 17, 33), ids=5, void=0.1):
    """ids 0..ids - 1 (so object `ids` is absent from both), `void` of b's pixels 255"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, ids, shape).astype(np.uint8)
    b = rng.integers(0, ids, shape).astype(np.uint8)
    b[rng.random(shape) < void] = 255
    return a, b


def test_restatement_properties():
    """what the issue states about the restatement: the sum, the marginals, and rmem_mask_iou_counts' numbers for every pair"""
    a, b = _stacks()
    n, H, W = a.shape
    C = pair_ref.census(a, b, 5, 5).astype(np.int64)
    assert C.sum() == n * H * W and (C.sum(axis=(1, 2)) == H * W).all()
    for v in range(6):
        assert np.array_equal(C[:, v, :].sum(axis=1), (a == v).sum(axis=(1, 2)))
        assert np.array_equal(C[:, :, v].sum(axis=1), (b == v).sum(axis=(1, 2)))
    assert np.array_equal(C[:, :, 6].sum(axis=1), (b == 255).sum(axis=(1, 2))) and not C[:, 6].any()
    D = C[:, :, :-1]
    for f in range(n):
        ok = b[f] != 255
        for i in range(1, 6):
            for j in range(1, 6):
                assert D[f, i, j] == np.count_nonzero((a[f] == i) & (b[f] == j) & ok)
                assert D[f, i].sum() + D[f, :, j].sum() - D[f, i, j] == np.count_nonzero(((a[f] == i) | (b[f] == j)) & ok)


# ------------------------------------------------------------------------------------------------------------ iou from tables
@pytest.mark.parametrize('drop', [True, False])
def test_pair_iou_and_track_iou_equal_the_mask_definitions(drop):
    import torch
    from rmem_ocu_amd import pairs
    a, b = _stacks()
    C = pair_ref.census(a, b, 5, 5)
    iou, inter, union = pairs.pair_iou(C, drop_other_b=drop)
    w_iou, w_inter, w_union = pair_ref.pair_iou(a, b, 5, 5, drop)
    assert iou.dtype == np.float64 and inter.dtype == np.int64 and union.dtype == np.int64 and iou.shape == (3, 5, 5)
    assert np.array_equal(inter, w_inter) and np.array_equal(union, w_union)
    assert np.array_equal(iou, w_iou, equal_nan=True)
    assert np.isnan(iou[:, 4, 4]).all() and not np.isnan(iou[:, :4, :4]).any()      # object 5 is absent from both
    if drop:
        full = pairs.pair_iou(C, drop_other_b=False)[2]
        assert (full[:, :4, :4] > union[:, :4, :4]).all(), 'void pixels count nowhere'
    assert np.array_equal(pairs.pair_iou(torch.from_numpy(C), drop)[0], iou, equal_nan=True)        # a tensor is accepted
    for frames, rows in ((None, None), ([0, 2], [0, 2]), (slice(1, None), [1, 2]), ([1], [1])):
        got = pairs.track_iou(C, frames, drop_other_b=drop)
        want = pair_ref.track_iou(a, b, 5, 5, rows, drop)
        assert got.dtype == np.float64 and got.shape == (5, 5) and np.array_equal(got, want), frames
        assert (got[4] == 0).all() and (got[:, 4] == 0).all() and (got[:4, :4] > 0).all()


def test_rectangular_tables():
    from rmem_ocu_amd import pairs
    a, b = _stacks(seed=9, shape=(2, 9, 14), ids=7)
    C = pair_ref.census(a, b, 6, 3)
    iou, inter, union = pairs.pair_iou(C)
    w = pair_ref.pair_iou(a, b, 6, 3)
    assert iou.shape == (2, 6, 3) and np.array_equal(inter, w[1]) and np.array_equal(union, w[2]) and np.array_equal(iou, w[0], equal_nan=True)
    assert np.array_equal(pairs.track_iou(C), pair_ref.track_iou(a, b, 6, 3))


# ------------------------------------------------------------------------------------------------------------------ assign
def _random_scores(rng):
    """multiples of 1/8 from a small range: ties are frequent, sums are exact, some entries are zero or negative"""
    R, C = (int(v) for v in rng.integers(1, 7, 2))
    return rng.integers(-2, 7, (R, C)) / 8.0


def test_assign_equals_brute_force():
    from rmem_ocu_amd import pairs
    rng = np.random.default_rng(2024)
    shapes = set()
    for k in range(200):
        s = _random_scores(rng)
        if k % 5 == 0:
            s = s[:min(s.shape), :min(s.shape)]                    # square ones as well
        shapes.add(s.shape)
        for minimum in (0.0, 0.25, -1.0):
            want, total = pair_ref.assign(s, minimum)
            got = pairs.assign(s, minimum)
            assert got == want, (s.tolist(), minimum)
            if minimum == -1.0:                                     # nothing is left out: the list is a full assignment
                assert len(got) == min(s.shape) and sum(s[i, j] for i, j in got) == total
            assert all(s[i, j] > minimum for i, j in got)
    assert any(r < c for r, c in shapes) and any(r > c for r, c in shapes) and any(r == c for r, c in shapes)


def test_assign_tie_rule():
    from rmem_ocu_amd import pairs
    assert pairs.assign([[1, 1], [1, 1]]) == [(0, 0), (1, 1)]
    assert pairs.assign([[1, 2], [2, 3]]) == [(0, 0), (1, 1)]       # 1 + 3 == 2 + 2
    assert pairs.assign([[2, 1], [3, 2], [9, 0]]) == [(1, 1), (2, 0)]                 # no tie: 9 + 2, row 0 stays without a column
    assert pairs.assign([[0, 0], [0, 0], [1, 1]]) == [(2, 1)]       # the full list [(0, 0), (2, 1)] is the smallest; zeros are left out
    assert pairs.assign([[0, 0], [0, 0]]) == [] and pairs.assign([[0, 0], [0, 0]], minimum=-1.0) == [(0, 0), (1, 1)]
    assert pairs.assign([[0.5]], minimum=0.5) == [] and pairs.assign([[0.5]], minimum=0.25) == [(0, 0)]
    s = np.array([[1, 1, 0], [1, 0, 0], [0, 1, 1]]) / 4.0           # row 0 cannot have column 0: row 1 has nothing else
    assert pairs.assign(s) == [(0, 1), (1, 0), (2, 2)]
    s = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]]) / 4.0           # rows 0 and 1 may trade columns
    assert pairs.assign(s) == [(0, 0), (1, 1), (2, 2)]
    assert pairs.assign(np.zeros((255, 255))) == [] and pairs.assign(np.eye(255)[::-1]) == [(i, 254 - i) for i in range(255)]


def test_assign_totals_equal_scipy():
    optimize = pytest.importorskip('scipy.optimize')
    from rmem_ocu_amd import pairs
    rng = np.random.default_rng(31)
    for R, C in ((1, 1), (4, 4), (7, 3), (3, 9), (20, 20), (33, 60), (60, 33)):
        s = rng.integers(0, 1 << 20, (R, C)) / float(1 << 20)       # sums of a few hundred such values are exact
        rows, cols = optimize.linear_sum_assignment(s, maximize=True)
        got = pairs.assign(s, minimum=-1.0)
        assert len(got) == min(R, C) and len({i for i, _ in got}) == len({j for _, j in got}) == len(got)
        assert sum(s[i, j] for i, j in got) == s[rows, cols].sum(), (R, C)


def test_package_does_not_import_scipy():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rmem_ocu_amd', 'pairs.py')).read()
    assert 'scipy' not in src


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_entry_point_refuses_on_the_host(lib):
    """non-zero, a message, nothing launched (there is no GPU in this tier)"""
    fake = 4096                                                     # a non-null address that is never dereferenced on the host
    for args, word in (((None, fake, 1, 4, 4, 3, 3, fake, None), b'null'), ((fake, None, 1, 4, 4, 3, 3, fake, None), b'null'),
                       ((fake, fake, 1, 4, 4, 3, 3, None, None), b'null'),
                       ((fake, fake, 0, 4, 4, 3, 3, fake, None), b'1..65535'), ((fake, fake, 65536, 4, 4, 3, 3, fake, None), b'1..65535'),
                       ((fake, fake, 1, 0, 4, 3, 3, fake, None), b'positive'), ((fake, fake, 1, 4, -1, 3, 3, fake, None), b'positive'),
                       ((fake, fake, 1, 8193, 8193, 3, 3, fake, None), b'2^26'),
                       ((fake, fake, 1, 4, 4, 0, 3, fake, None), b'1..255'), ((fake, fake, 1, 4, 4, 256, 3, fake, None), b'1..255'),
                       ((fake, fake, 1, 4, 4, 3, 0, fake, None), b'1..255'), ((fake, fake, 1, 4, 4, 3, 256, fake, None), b'1..255'),
                       ((fake, fake, 1, 4, 4, -5, 3, fake, None), b'1..255')):
        rc = lib.rmem_label_pair_census(*args)
        msg = lib.rmem_last_error_string()
        assert rc != 0 and b'rmem_label_pair_census' in msg and word in msg, (args, msg)


def test_lds_constant(lib):
    bins = lib.rmem_label_pair_census_lds_bins()
    assert bins > 0 and bins % 64 == 0 and bins <= 40960
    assert lib.rmem_abi_version() == 15


def test_python_refusals():
    import torch
    from rmem_ocu_amd import pairs
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import identity_report, relabel_to_match
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(RmemError, match='device tensor'):
        pairs.pair_census(x, x, 3, 3)
    with pytest.raises(RmemError, match='device tensor'):
        relabel_to_match(x, x, 3, 3)
    with pytest.raises(RmemError, match='device tensor'):
        identity_report(x, x, 3)
    with pytest.raises(RmemError, match='void_label'):
        identity_report(x, x, 255)
    for bad in (0, 256, -1, 2.5, None, True):
        with pytest.raises(RmemError, match=r'num_a must be an integer in 1\.\.255'):
            pairs.pair_census(x, x, bad, 3)
        with pytest.raises(RmemError, match=r'num_b must be an integer in 1\.\.255'):
            pairs.pair_census(x, x, 3, bad)
    for fn in (pairs.pair_iou, pairs.track_iou):
        with pytest.raises(RmemError, match='census'):
            fn(np.zeros((3, 3), dtype=np.int32))
        with pytest.raises(RmemError, match='census'):
            fn(np.zeros((1, 2, 3), dtype=np.int32))
        with pytest.raises(RmemError, match='census'):
            fn(np.zeros((1, 3, 3)))
    with pytest.raises(RmemError, match='finite'):
        pairs.assign([[0.5, float('nan')]])
    with pytest.raises(RmemError, match='finite'):
        pairs.assign([[float('inf')]])
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((256, 2)), np.zeros((2, 256))):
        with pytest.raises(RmemError, match='matrix'):
            pairs.assign(bad)
