"""Clip scoring, host side (no GPU): the numpy restatement's dilation against the definition, rmem_boundary_radius and
rmem_clip_score_workspace_bytes, the argument checks of rmem_clip_score_counts, and evaluator.scores_from_counts /
summarize_scores against the restatement on hand-made counts."""
import math
import os

import numpy as np
import pytest

import boundary_ref as R


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_restatement_dilation_equals_brute_force():
    lab = R.blobs(40, 50, 5, seed=2)
    for k, r in ((1, 1), (2, 3), (3, 8)):
        b = R.seg2bmap(lab == k)
        assert b.any()
        assert np.array_equal(R.dilate(b, r), R.dilate_brute(b, r))
    edge = np.zeros((40, 50), bool)
    edge[0, 0] = edge[39, 49] = edge[20, 49] = True          # zero padding: nothing wraps or reflects at the border
    assert np.array_equal(R.dilate(edge, 5), R.dilate_brute(edge, 5))


def test_restatement_seg2bmap_edge_rules():
    m = np.zeros((4, 5), bool)
    m[2:, 3:] = True
    b = R.seg2bmap(m)
    want = np.zeros((4, 5), bool)
    want[1, 2:] = True            # differs from the south / south-east neighbour
    want[2, 2] = want[3, 2] = True
    assert np.array_equal(b, want)      # last row: east only; last column: south only; bottom-right: 0
    assert not R.seg2bmap(np.ones((4, 5), bool)).any()


@pytest.mark.parametrize('H,W,r', [(480, 854, 8), (1080, 1920, 18), (97, 131, 2), (64, 64, 1)])
def test_boundary_radius(lib, H, W, r):
    assert lib.rmem_boundary_radius(H, W, 0.008) == math.ceil(0.008 * math.sqrt(H * H + W * W)) == r == R.radius(H, W)
    assert lib.rmem_boundary_radius(H, W, 3.0) == 3
    assert lib.rmem_boundary_radius(H, W, 0.02) == math.ceil(0.02 * math.sqrt(H * H + W * W))


def test_boundary_radius_bad_arguments(lib):
    for args in ((0, 10, 0.008), (10, -1, 0.008), (10, 10, 0.0), (10, 10, -1.0), (10, 10, float('nan')), (10, 10, 2.5)):
        assert lib.rmem_boundary_radius(*args) == -1


def test_workspace_bytes(lib):
    f = lib.rmem_clip_score_workspace_bytes
    assert f(1, 480, 854, 11) == 2 * 11 * 480 * 14 * 8
    assert 0 < f(1, 40, 50, 2) < f(2, 40, 50, 2) < f(2, 40, 50, 3) < f(2, 40, 65, 3)
    assert f(64, 1080, 1920, 32) == 64 * 2 * 32 * 1080 * 30 * 8            # beyond 2^32: size_t arithmetic
    for bad in ((0, 40, 50, 5), (1, 0, 50, 5), (1, 40, 0, 5), (1, 40, 50, 1), (1, 40, 50, 33)):
        assert f(*bad) == 0


def test_counts_argument_checks_need_no_gpu(lib):
    call = lib.rmem_clip_score_counts
    for radius, word in ((0, b'radius'), (64, b'radius')):
        assert call(None, None, 1, 40, 50, 5, 255, radius, None, None, None) != 0
        assert word in lib.rmem_last_error_string()
    for ids in (1, 33):
        assert call(None, None, 1, 40, 50, ids, 255, 2, None, None, None) != 0
        assert b'num_ids' in lib.rmem_last_error_string()
    for frames, H, W in ((0, 40, 50), (1, 0, 50), (1, 40, -3)):
        assert call(None, None, frames, H, W, 5, 255, 2, None, None, None) != 0
        assert b'positive' in lib.rmem_last_error_string()
    assert call(None, None, 1, 40, 50, 5, 255, 2, None, None, None) != 0        # everything in range, null pointers
    assert b'null' in lib.rmem_last_error_string()


def hand_made_counts():
    """[5 frames, 4 ids, 6]: every f_measure edge case, an object (id 2) that vanishes mid-clip, exact and zero matches"""
    c = np.zeros((5, 4, 6), np.int64)
    c[0, 1] = [100, 90, 80, 60, 900, 1000]       # the general case
    c[1, 1] = [100, 90, 0, 0, 0, 1900]           # boundaries on both sides, nothing matched: P + R = 0 -> F = 0
    c[2, 1] = [57, 57, 57, 57, 400, 400]         # perfect
    c[3, 1] = [0, 40, 0, 0, 0, 300]              # no prediction boundary: P = 1, R = 0
    c[4, 1] = [35, 0, 0, 0, 0, 250]              # no annotation boundary: P = 0, R = 1
    c[0, 2] = [30, 33, 29, 30, 200, 260]
    c[1, 2] = [28, 31, 11, 12, 90, 300]
    c[2, 2] = [0, 0, 0, 0, 0, 0]                 # gone from both: P = R = 1, J = 1
    c[3, 2] = [0, 0, 0, 0, 0, 0]
    c[4, 2] = [12, 0, 0, 0, 0, 9]                # predicted again, not annotated
    c[:, 3] = [[10, 10, 7, 3, 50, 70], [0, 0, 0, 0, 640, 640], [9, 12, 9, 0, 1, 99], [9, 12, 0, 12, 30, 60], [1, 1, 1, 1, 1, 1]]
    return c


def test_scores_from_counts():
    from rmem_ocu_amd import evaluator
    c = hand_made_counts()
    J, F = evaluator.scores_from_counts(c)
    Jr, Fr = R.scores(c)
    assert J.dtype == np.float64 and J.shape == (5, 4)
    assert np.abs(J - Jr).max() < 1e-15 and np.abs(F - Fr).max() < 1e-15
    assert F[1, 1] == 0.0 and F[2, 1] == 1.0 and F[3, 1] == 0.0 and F[4, 1] == 0.0 and F[2, 2] == 1.0 and J[2, 2] == 1.0
    assert J[4, 2] == 0.0 and F[1, 3] == 1.0 and J[1, 3] == 1.0      # a full-frame object: no boundary on either side, J = 1
    assert abs(F[0, 1] - 2 * 0.8 * (60 / 90) / (0.8 + 60 / 90)) < 1e-15
    assert (J[:, 0] == 1.0).all() and (F[:, 0] == 1.0).all()         # the zero row of id 0


@pytest.mark.parametrize('frames,tail', [(slice(1, -1), 0.25), (slice(0, None), 0.25), (slice(0, None), 0.5), ([0, 2, 3, 4], 1.0)])
def test_clip_summary_five_frames(frames, tail):
    from rmem_ocu_amd import evaluator
    J, F = R.scores(hand_made_counts())
    got = evaluator.summarize_scores(J[:, 1:], F[:, 1:], frames, tail)
    want = R.summary(J[:, 1:], F[:, 1:], frames, tail)
    for name, v in want.items():
        assert np.abs(np.asarray(getattr(got, name)) - np.asarray(v)).max() < 1e-15, name
    assert abs(got.JF_mean - 0.5 * (got.J_mean + got.F_mean)) < 1e-15
    assert got.J.shape == (5, 3) and list(got.frames) == list(np.arange(5)[frames])


def test_sequence_statistics_long_clip():
    """decay bins of a 50-frame object: edges round(linspace(1, 50, 5) + 1e-10) - 1 = 0, 12, 24, 37, 49, both ends included"""
    from rmem_ocu_amd import evaluator
    v = np.linspace(1.0, 0.2, 50)
    mean, recall, decay = evaluator.sequence_statistics(v)
    assert abs(mean - v.mean()) < 1e-15 and abs(recall - (v > 0.5).mean()) < 1e-15
    assert abs(decay - (v[0:13].mean() - v[37:50].mean())) < 1e-15
    assert all(abs(a - b) < 1e-15 for a, b in zip((mean, recall, decay), R.db_statistics(v)))
    for n in (1, 2, 3, 4):
        assert all(abs(a - b) < 1e-15 for a, b in zip(evaluator.sequence_statistics(v[:n]), R.db_statistics(v[:n])))


def test_host_tensors_are_refused():
    import torch
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    x = torch.zeros(3, 8, 8, dtype=torch.uint8)
    for fn, a in ((evaluator.clip_counts, x), (evaluator.boundary_accuracy, x[0]), (evaluator.score_clip, x)):
        with pytest.raises(RmemError, match='device'):
            fn(a, a)
    with pytest.raises(RmemError, match='no frame'):
        evaluator.summarize_scores(np.ones((2, 1)), np.ones((2, 1)))
