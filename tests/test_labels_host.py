"""Host checks the modules on label stacks share (rmem_ocu_amd._labels): the workspace budget, integers in a range, connectivity,
the keys of un-squeezed objects, and the one copy of the boundary P / R / F behind evaluator.scores_from_counts and pairs.pair_f.
No GPU."""
import numpy as np
import pytest

NOUNS = ("one frame's planes", "one frame's need")


def test_frames_per_pass():
    from rmem_ocu_amd import _labels
    from rmem_ocu_amd._lib import RmemError
    cap = _labels.WORKSPACE_CAP
    assert cap == 256 << 20
    for noun in NOUNS:
        assert _labels.frames_per_pass('m.f', 5, 100, None, noun) == (max(100, min(500, cap)), 5) == (500, 5)
        assert _labels.frames_per_pass('m.f', 5, 100, 100, noun) == (100, 1)
        assert _labels.frames_per_pass('m.f', 5, 100, 201, noun) == (201, 2)
        assert _labels.frames_per_pass('m.f', 5, 100, 10 ** 9, noun) == (10 ** 9, 5)
        assert _labels.frames_per_pass('m.f', 5, 100, np.int64(300), noun) == (300, 3)
        assert _labels.frames_per_pass('m.f', 5, cap + 16, None, noun) == (cap + 16, 1)       # one frame's bytes above the cap
        assert _labels.frames_per_pass('m.f', 10 ** 4, 10 ** 6, None, noun) == (cap, cap // 10 ** 6)
        for bad in (99, True, 100.0):
            with pytest.raises(RmemError) as e:
                _labels.frames_per_pass('m.f', 5, 100, bad, noun)
            assert str(e.value) == f'm.f: workspace_bytes must be an integer of at least {noun}, 100 bytes (got {bad!r})'


def test_int_in_and_connectivity():
    from rmem_ocu_amd import _labels
    from rmem_ocu_amd._lib import RmemError
    got = _labels.int_in('m.f', 'num_objs', np.int64(3), 1, 255)
    assert got == 3 and type(got) is int
    got = _labels.connectivity('m.f', np.int32(8))
    assert got == 8 and type(got) is int
    assert _labels.int_in('m.f', 'num_objs', 255, 1, 255) == 255 and _labels.connectivity('m.f', 4) == 4
    for bad in (True, 0, 256, 1.0, '8', 6.5, None):
        with pytest.raises(RmemError) as e:
            _labels.int_in('m.f', 'num_a', bad, 1, 255)
        assert str(e.value) == f'm.f: num_a must be an integer in 1..255 (got {bad!r})'
        with pytest.raises(RmemError) as e:
            _labels.int_in('m.f', 'num_objs', bad, 1, 255, must_be='in')
        assert str(e.value) == f'm.f: num_objs must be in 1..255 (got {bad!r})'
    assert _labels.int_in('m.f', 'num_objs', 6, 1, 255) == 6
    for bad in (True, 0, 256, 1.0, '8', 6):
        with pytest.raises(RmemError) as e:
            _labels.connectivity('m.f', bad)
        assert str(e.value) == f'm.f: connectivity must be 4 or 8 (got {bad!r})'


def test_object_keys():
    from rmem_ocu_amd import _labels
    assert _labels.object_keys(4) == {1: 1, 2: 2, 3: 3, 4: 4}
    assert list(_labels.object_keys(4)) == [1, 2, 3, 4]
    keys = _labels.object_keys(4, np.array([0, 7, 9], dtype=np.uint8))             # shorter than K + 1: ids 3 and 4 are left out
    assert keys == {1: 7, 2: 9} and all(type(v) is int for v in keys.values())
    assert _labels.object_keys(2, [0, 7, 9, 11, 13]) == {1: 7, 2: 9}
    assert _labels.object_keys(3, [0]) == {}


def test_boundary_prf_is_the_one_copy():
    """rows: no boundary in a, none in b, neither, both without a match (P + R = 0), a generic pair -- the constants of
    _labels.boundary_prf's docstring"""
    from rmem_ocu_amd import _labels, pairs
    from rmem_ocu_amd.evaluator import scores_from_counts
    rows = np.array([[0, 7, 0, 0], [6, 0, 0, 0], [0, 0, 0, 0], [3, 5, 0, 0], [4, 8, 2, 2]], dtype=np.int64)   # n_fg, n_gt, fg_m, gt_m
    want = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.5, 0.25, 1 / 3]])
    P, R, F = _labels.boundary_prf(*(rows[:, i].astype(np.float64) for i in range(4)))
    assert np.array_equal(np.stack([P, R, F], axis=1), want)
    K = len(rows)
    counts = np.zeros((1, K, 6), dtype=np.int64)
    counts[0, :, :4] = rows
    match = np.zeros((1, K + 1, K + 1, 2), dtype=np.int32)
    match[..., 0], match[..., 1] = 1000, 2000                                    # off the diagonal: nothing the diagonal may read
    d = np.arange(1, K + 1)
    match[0, d, d, 0], match[0, d, d, 1] = rows[:, 2], rows[:, 3]
    bnd_a, bnd_b = np.zeros((1, K + 1), dtype=np.int32), np.zeros((1, K + 1), dtype=np.int32)
    bnd_a[0, 1:], bnd_b[0, 1:] = rows[:, 0], rows[:, 1]
    from_pairs = pairs.pair_f(match, bnd_a, bnd_b)[:, d - 1, d - 1]
    from_counts = scores_from_counts(counts)[1]
    assert from_pairs.dtype == from_counts.dtype == np.float64
    assert np.array_equal(from_pairs, from_counts)
    assert np.array_equal(from_counts[0], want[:, 2])
