"""The pair boundary census without a GPU: the restatement (tests/pair_boundary_ref.py) against tables written out by hand and
against boundary_ref, its dilation against scipy's and against the definition, pairs.pair_f against f_measure's last lines, the
host half of the unsupervised protocol against trying every assignment, and every refusal that is raised on the host."""
import os

import numpy as np
import pytest

import boundary_ref
import pair_boundary_ref as ref


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_against_tables_by_hand():
    """3 x 4, object 1 = the left two columns, object 2 = the right two, on both sides; r = 1.
    seg2bmap of the left half: rows 0..2 of column 1 (each differs from its east neighbour; the last row compares east only);
    column 0 never differs -> 3 boundary pixels, at x = 1.  Of the right half: column 1 again (the boundary is marked on the
    north-west pixel of a change, which lies in the other object) -> the same 3 pixels.  So every boundary is column 1, dilated by
    one pixel it is columns 0..2, and every pair matches all 3 pixels both ways."""
    a = np.array([[1, 1, 2, 2]] * 3, dtype=np.uint8)
    match, bnd_a, bnd_b = ref.frame_tables(a, a, 2, 2, 255, 1)
    assert bnd_a.tolist() == [0, 3, 3] and bnd_b.tolist() == [0, 3, 3]
    want = np.zeros((3, 3, 2), dtype=np.int64)
    want[1:, 1:] = 3
    assert np.array_equal(match, want)
    # b's objects moved two pixels right: B_1 = columns 0..3 is the whole frame (no boundary), B_2 is absent
    b = np.array([[1, 1, 1, 1]] * 3, dtype=np.uint8)
    match, bnd_a, bnd_b = ref.frame_tables(a, b, 2, 2, 255, 1)
    assert bnd_a.tolist() == [0, 3, 3] and bnd_b.tolist() == [0, 0, 0] and not match.any()
    # b = object 1 in column 3 only: its boundary is column 2 (rows 0..2) plus nothing in column 3 (the last column compares
    # south only, and the column is uniform) -> 3 pixels at x = 2; a's boundaries at x = 1 are one pixel away: all match at r = 1
    b = np.array([[0, 0, 0, 1]] * 3, dtype=np.uint8)
    match, bnd_a, bnd_b = ref.frame_tables(a, b, 2, 1, 255, 1)
    assert bnd_b.tolist() == [0, 3]
    assert match[1:, 1].tolist() == [[3, 3], [3, 3]] and not match[0].any() and not match[:, 0].any()


def test_restatement_with_void_by_hand():
    """The frame of the first table with b's column 1 void: A_1 = column 0 only, whose boundary is column 0 (its east neighbour is
    "not 1"), A_2 = columns 2..3, boundary column 1 as before -- void pixels are "not the object", they still carry boundary marks.
    B_1 = column 0: boundary column 0.  B_2 = columns 2..3: boundary column 1."""
    a = np.array([[1, 1, 2, 2]] * 3, dtype=np.uint8)
    b = np.array([[1, 255, 2, 2]] * 3, dtype=np.uint8)
    match, bnd_a, bnd_b = ref.frame_tables(a, b, 2, 2, 255, 1)
    assert bnd_a.tolist() == [0, 3, 3] and bnd_b.tolist() == [0, 3, 3]
    assert match[1, 1].tolist() == [3, 3] and match[2, 2].tolist() == [3, 3]         # the same column on both sides
    assert match[1, 2].tolist() == [3, 3] and match[2, 1].tolist() == [3, 3]         # columns 0 and 1 are one pixel apart
    # without the void rule a's object 1 keeps column 1 and b's column 1 is no object: A_1's boundary moves to column 1
    match, bnd_a, bnd_b = ref.frame_tables(a, b, 2, 2, None, 1)
    assert bnd_a.tolist() == [0, 3, 3] and match[1, 1].tolist() == [3, 3]
    # two pixels apart at r = 1: b's only object in column 3 against a's column-0 object under void
    a2 = np.array([[1, 0, 0, 0]] * 3, dtype=np.uint8)
    b2 = np.array([[0, 0, 0, 1]] * 3, dtype=np.uint8)
    match, bnd_a, bnd_b = ref.frame_tables(a2, b2, 1, 1, 255, 1)
    assert bnd_a.tolist() == [0, 3] and bnd_b.tolist() == [0, 3] and match[1, 1].tolist() == [0, 0]
    match, _, _ = ref.frame_tables(a2, b2, 1, 1, 255, 2)
    assert match[1, 1].tolist() == [3, 3]


def test_restatement_diagonal_equals_boundary_ref():
    a = boundary_ref.blobs(37, 131, 6, seed=3)
    b = boundary_ref.shifted_speckled(a, 2, 3, seed=3)
    b[5:9, 20:40] = 255
    got = ref.tables(a[None], b[None], 5, 5, 255, 3)
    want = boundary_ref.frame_counts(a, b, 6, 255, 3)
    d = np.arange(6)
    assert np.array_equal(got[1][0], want[:, 0]) and np.array_equal(got[2][0], want[:, 1])
    assert np.array_equal(got[0][0, d, d, 0], want[:, 2]) and np.array_equal(got[0][0, d, d, 1], want[:, 3])
    # values above num are "not the object", on both sides
    got3 = ref.tables(a[None], b[None], 3, 2, 255, 3)
    assert np.array_equal(got3[0][0], got[0][0, :4, :3]) and np.array_equal(got3[1][0], got[1][0, :4])


def test_dilation_equals_scipy_and_the_definition():
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (1, 17), (3, 5), (17, 33), (37, 131)):
        for r in (1, 2, 3, 8, 20):
            for density in (0.002, 0.05):
                m = rng.random((H, W)) < density
                m[rng.integers(H), rng.integers(W)] = True
                assert np.array_equal(ref.dilate(m, r), boundary_ref.dilate(m, r)), (H, W, r)
    for H, W in ((1, 1), (2, 3), (5, 9), (9, 14)):
        for r in (1, 2, 3, 5):
            m = rng.random((H, W)) < 0.15
            assert np.array_equal(ref.dilate(m, r), boundary_ref.dilate_brute(m, r)), (H, W, r)
    assert not ref.dilate(np.zeros((4, 5), dtype=bool), 3).any()


def test_dilation_at_radius_63():
    rng = np.random.default_rng(6)
    m = np.zeros((150, 200), dtype=bool)
    m[rng.integers(0, 150, 4), rng.integers(0, 200, 4)] = True
    assert np.array_equal(ref.dilate(m, 63), boundary_ref.dilate(m, 63))


# --------------------------------------------------------------------------------------------------------------------- pair_f
def test_pair_f_equals_f_measure_element_by_element():
    from rmem_ocu_amd import pairs
    rng = np.random.default_rng(7)
    n, na, nb = 3, 4, 5
    bnd_a = rng.integers(1, 50, (n, na + 1))
    bnd_b = rng.integers(1, 50, (n, nb + 1))
    bnd_a[:, 0] = bnd_b[:, 0] = 0
    bnd_a[0, 1] = bnd_a[1, 2] = bnd_b[0, 1] = bnd_b[2, 3] = 0         # absent boundaries: the edge cases, three of them on frame 0
    match = np.zeros((n, na + 1, nb + 1, 2), dtype=np.int64)
    match[..., 0] = rng.integers(0, 51, match.shape[:3]) % (bnd_a[:, :, None] + 1)
    match[..., 1] = rng.integers(0, 51, match.shape[:3]) % (bnd_b[:, None, :] + 1)
    match[bnd_a[:, :, None] * bnd_b[:, None, :] == 0] = 0
    match[0, 3, 3] = 0                                                  # both boundaries there, nothing matched: P + R = 0
    got = pairs.pair_f(match.astype(np.int32), bnd_a.astype(np.int32), bnd_b.astype(np.int32))
    want = ref.f_table(match, bnd_a, bnd_b)
    assert got.dtype == np.float64 and got.shape == (n, na, nb)
    assert np.array_equal(got, want)
    assert got[0, 0, 0] == 1.0 and got[0, 0, 1] == 0.0 and got[0, 1, 0] == 0.0 and got[0, 2, 2] == 0.0
    assert bnd_a[0, 3] > 0 and bnd_b[0, 3] > 0


def test_jf_from_tables_fills_the_empty_union():
    from rmem_ocu_amd import pairs
    census = np.zeros((1, 4, 4), dtype=np.int32)                       # 2 x 2 objects + background + other
    census[0, 0, 0], census[0, 1, 1], census[0, 1, 3] = 10, 4, 2       # object 1 on object 1, and on two void pixels
    z = np.zeros((1, 3), dtype=np.int32)
    J, F = pairs.jf_from_tables(census, np.zeros((1, 3, 3, 2), dtype=np.int32), z, z)
    assert J[0].tolist() == [[1.0, 0.0], [0.0, 1.0]] and (F == 1.0).all()
    J, _ = pairs.jf_from_tables(census, np.zeros((1, 3, 3, 2), dtype=np.int32), z, z, drop_other_b=False)
    assert J[0, 0, 0] == 4 / 6


# ------------------------------------------------------------------------------------------------- the unsupervised host half
def _series(rng, n, R, C):
    J, F = rng.random((n, R, C)), rng.random((n, R, C))
    area = rng.integers(0, 2, (n, C)) * 7
    bnd = np.where(area > 0, rng.integers(0, 2, (n, C)) * 3, 0)
    return J, F, area, bnd


@pytest.mark.parametrize('R,C', [(1, 1), (2, 2), (4, 4), (2, 4), (3, 4), (4, 2), (4, 3), (1, 3), (3, 1)])
def test_unsupervised_host_half_equals_every_assignment(R, C):
    from rmem_ocu_amd.evaluator import summarize_scores, summarize_unsupervised
    rng = np.random.default_rng(100 * R + C)
    n = 6
    J, F, area, bnd = _series(rng, n, R, C)
    if C > 1:                                                           # an object absent from every frame
        area[:, C - 1] = bnd[:, C - 1] = 0
    for frames in (slice(None), slice(1, -1)):
        score, mapping = summarize_unsupervised(J, F, area, bnd, frames)
        best, hits = ref.unsupervised_brute(J, F, area, bnd, frames)
        assert len(hits) == 1, 'random series do not tie'
        want = {j + 1: (hits[0][j] + 1 if j in hits[0] else None) for j in range(C)}
        assert mapping == want
        assert sum(v is not None for v in mapping.values()) == min(R, C)
        Jw, Fw = np.zeros((n, C)), np.zeros((n, C))
        for j in range(C):
            i = hits[0].get(j)
            for t in range(n):
                Jw[t, j] = J[t, i, j] if i is not None else (1.0 if area[t, j] == 0 else 0.0)
                Fw[t, j] = F[t, i, j] if i is not None else boundary_ref.f_from_counts(0, int(bnd[t, j]), 0, 0)
        assert np.array_equal(score.J, Jw) and np.array_equal(score.F, Fw)
        ws = summarize_scores(Jw, Fw, frames, 0.25)
        assert score.JF_mean == ws.JF_mean and np.array_equal(score.J_obj_mean, ws.J_obj_mean)
        want_sum = boundary_ref.summary(Jw, Fw, frames)
        assert np.allclose(score.JF_mean, want_sum['JF_mean'], rtol=0, atol=1e-15)


def test_unsupervised_keeps_a_partner_that_never_overlaps():
    """M = 0 is still an assignment: the object is scored by its partner, not against an empty prediction"""
    from rmem_ocu_amd.evaluator import summarize_unsupervised
    J, F = np.zeros((2, 1, 1)), np.zeros((2, 1, 1))
    score, mapping = summarize_unsupervised(J, F, np.array([[0], [5]]), np.array([[0], [3]]))
    assert mapping == {1: 1} and not score.J.any()


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_workspace_bytes(lib):
    f = lib.rmem_pair_boundary_workspace_bytes
    # 3 frames of 37 x 131 with 5 + 3 ids: 3 words per row, (5 + 3 + 2) planes of 37 * 3 words of 8 bytes
    assert f(3, 37, 131, 5, 3) == 3 * 10 * 37 * 3 * 8 == 26640
    assert f(1, 1080, 1920, 255, 255) == 512 * 1080 * 30 * 8
    for bad in ((0, 4, 4, 1, 1), (65536, 4, 4, 1, 1), (1, 0, 4, 1, 1), (1, 4, -1, 1, 1), (1, 8193, 8193, 1, 1), (1, 4, 4, 0, 1),
                (1, 4, 4, 256, 1), (1, 4, 4, 1, 0), (1, 4, 4, 1, 256)):
        assert f(*bad) == 0, bad
    assert lib.rmem_abi_version() == 15


def test_entry_point_refuses_on_the_host(lib):
    """non-zero, a message, nothing launched (there is no GPU in this tier)"""
    fake = 4096                                                     # a non-null, aligned address that is never dereferenced on the host
    big = 1 << 30

    def args(a=fake, b=fake, frames=1, H=4, W=4, num_a=3, num_b=3, void=255, radius=2, ws=fake, ws_bytes=big, bnd_a=fake, bnd_b=fake,
             match=fake):
        return (a, b, frames, H, W, num_a, num_b, void, radius, ws, ws_bytes, bnd_a, bnd_b, match, None)

    one_frame = lib.rmem_pair_boundary_workspace_bytes(1, 4, 4, 3, 3)
    assert one_frame == 8 * 4 * 8
    cases = [(dict(a=None), b'null'), (dict(b=None), b'null'), (dict(ws=None), b'null'), (dict(bnd_a=None), b'null'),
             (dict(bnd_b=None), b'null'), (dict(match=None), b'null'),
             (dict(num_a=0), b'1..255'), (dict(num_a=256), b'1..255'), (dict(num_b=0), b'1..255'), (dict(num_b=256), b'1..255'),
             (dict(radius=0), b'1..63'), (dict(radius=64), b'1..63'), (dict(radius=-1), b'1..63'),
             (dict(frames=0), b'1..65535'), (dict(frames=65536), b'1..65535'),
             (dict(H=0), b'positive'), (dict(W=-1), b'positive'), (dict(H=8193, W=8193), b'2^26'),
             (dict(void=3), b'void_label'), (dict(void=0), b'void_label'), (dict(void=2), b'void_label'),
             (dict(num_b=255, void=255), b'void_label'),
             (dict(ws_bytes=one_frame - 1), b'smaller than one frame'), (dict(ws_bytes=0), b'smaller than one frame'),
             (dict(ws=fake + 4), b'aligned')]
    for kw, word in cases:
        rc = lib.rmem_pair_boundary_counts(*args(**kw))
        msg = lib.rmem_last_error_string()
        assert rc != 0 and b'rmem_pair_boundary_counts' in msg and word in msg, (kw, msg)


def test_python_refusals():
    import torch
    from rmem_ocu_amd import pairs
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import score_clip_objects, score_unsupervised_clip, summarize_unsupervised
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for fn in (pairs.pair_boundary_counts, pairs.pair_jf):
        with pytest.raises(RmemError, match='device tensor'):
            fn(x, x, 3, 3)
        with pytest.raises(RmemError, match='device tensor'):
            fn(x.float(), x, 3, 3)
        with pytest.raises(RmemError, match='device tensor'):
            fn(None, x, 3, 3)
        for bad in (0, 256, -1, 2.5, None, True):
            with pytest.raises(RmemError, match=r'num_a must be an integer in 1\.\.255'):
                fn(x, x, bad, 3)
            with pytest.raises(RmemError, match=r'num_b must be an integer in 1\.\.255'):
                fn(x, x, 3, bad)
    for bad in (3, 0, 256, 2.5, True):
        with pytest.raises(RmemError, match='void_label'):
            pairs.pair_boundary_counts(x, x, 3, 3, void_label=bad)
    with pytest.raises(RmemError, match='void_label'):
        pairs.pair_boundary_counts(x, x, 255, 255)
    with pytest.raises(RmemError, match='device tensor'):
        pairs.pair_boundary_counts(x, x, 255, 255, void_label=None)
    with pytest.raises(RmemError, match='device tensor'):
        score_clip_objects(x, x, 40)
    with pytest.raises(RmemError, match='max_proposals'):
        score_unsupervised_clip(x, x, 21, 3)
    with pytest.raises(RmemError, match='max_proposals'):
        score_unsupervised_clip(x, x, 3, 3, max_proposals=2)
    with pytest.raises(RmemError, match='device tensor'):
        score_unsupervised_clip(x, x, 20, 3)
    z = np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(RmemError, match='do not fit'):
        pairs.pair_f(np.zeros((2, 3, 4, 2), dtype=np.int32), z, z)
    with pytest.raises(RmemError, match='integer array'):
        pairs.pair_f(np.zeros((2, 3, 3, 2)), z, z)
    with pytest.raises(RmemError, match='integer array'):
        pairs.pair_f(np.zeros((2, 3, 3), dtype=np.int32), z, z)
    with pytest.raises(RmemError, match='num_gt'):
        summarize_unsupervised(np.zeros((2, 3, 3)), np.zeros((2, 3, 2)), z, z)
    with pytest.raises(RmemError, match='no frame'):
        summarize_unsupervised(np.zeros((2, 3, 3)), np.zeros((2, 3, 3)), z, z, frames=slice(1, -1))


def test_package_does_not_import_scipy():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rmem_ocu_amd', 'pairs.py')).read()
    assert 'scipy' not in src
