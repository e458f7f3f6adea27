"""The clip protocol without a GPU: protocol.protocol_from_census on a census equals the reference's curr_objs rule run directly
on the label maps (census_ref), its tables round-trip through png.squeeze_lut, the per-object score summary equals
summarize_scores where every object starts on frame 0 and census_ref elsewhere, and both C entry points refuse bad arguments on
the host."""
import os

import numpy as np
import pytest

import census_ref


def _stack(frames, H=6, W=8):
    """frames: per frame a list of (value, y, x) pixels, or of (value, y0, x0, y1, x1) boxes, on background 0"""
    a = np.zeros((len(frames), H, W), dtype=np.uint8)
    for f, items in enumerate(frames):
        for it in items:
            if len(it) == 3:
                a[f, it[1], it[2]] = it[0]
            else:
                a[f, it[1]:it[3], it[2]:it[4]] = it[0]
    return a


CASES = {
    'dense ids': (_stack([[(1, 0, 0), (2, 1, 1), (3, 2, 2)], [(1, 0, 1), (2, 1, 2), (3, 2, 3)]]), None),
    'sparse ids': (_stack([[(200, 0, 0), (3, 1, 1), (7, 2, 2)], [(7, 0, 1), (3, 1, 2)]]), None),
    'vanishes and returns': (_stack([[(5, 0, 0), (9, 1, 1)], [(9, 1, 1)], [(5, 3, 3), (9, 1, 1)], [(5, 3, 4)]]), None),
    'two enter on one later frame': (_stack([[(4, 0, 0)], [(4, 0, 0)], [(4, 0, 0), (90, 1, 1), (12, 5, 7)], [(12, 2, 2)]]), None),
    'annotated frame with nothing new': (_stack([[(4, 0, 0), (6, 1, 0)], [(6, 2, 2)], [(4, 1, 1), (8, 5, 5)], [(8, 0, 0)]]), None),
    'frame_index': (_stack([[(3, 0, 0)], [(3, 0, 1), (2, 4, 4)], [(2, 4, 5), (3, 0, 2), (250, 5, 0)]]), [0, 5, 9]),
    'void present': (_stack([[(1, 0, 0), (255, 2, 2, 4, 4)], [(1, 0, 0), (255, 1, 1), (2, 5, 5)]]), None),
    'void only later': (_stack([[(1, 0, 0)], [(1, 0, 0), (255, 1, 1), (2, 5, 5)]]), [0, 3]),
    '12 objects': (_stack([[(v, v % 6, v % 8) for v in (20, 21, 22, 23, 24, 25, 26)],
                           [(v, (v + 1) % 6, v % 8) for v in (20, 24, 27, 28, 2)], [(v, 0, v % 8) for v in (30, 29)]]), None),
}


def _check(labels, frame_index, void_label):
    from rmem_ocu_amd.protocol import protocol_from_census
    area = census_ref.census(labels)[:, :, 0]
    p = protocol_from_census(area, frame_index, void_label)
    squeeze_idx, first_frame, new_frames = census_ref.protocol(labels, frame_index, void_label)
    assert p.squeeze_idx == squeeze_idx
    assert p.num_objs == len(squeeze_idx) - 1
    assert p.first_frame.tolist() == first_frame
    assert p.new_frames == new_frames
    lut_all, lut_first, lut_new = census_ref.tables(squeeze_idx, first_frame, void_label)
    assert p.lut_all.dtype == np.uint8 and np.array_equal(p.lut_all, lut_all)
    assert p.lut_first.dtype == np.uint8 and np.array_equal(p.lut_first, lut_first)
    assert sorted(p.lut_new) == sorted(lut_new) == new_frames
    for t in new_frames:
        assert p.lut_new[t].dtype == np.uint8 and np.array_equal(p.lut_new[t], lut_new[t])
    # the tables give the overlays census_ref builds pixel set by pixel set
    idx = list(range(len(labels))) if frame_index is None else frame_index
    first, new = census_ref.overlays(labels, frame_index, void_label)
    assert np.array_equal(p.lut_first[labels[0]], first)
    for t in new_frames:
        assert np.array_equal(p.lut_new[t][labels[idx.index(t)]], new[t])
    return p


@pytest.mark.parametrize('void_label', [255, None])
@pytest.mark.parametrize('case', sorted(CASES))
def test_protocol_from_census_equals_the_direct_rule(case, void_label):
    labels, frame_index = CASES[case]
    p = _check(labels, frame_index, void_label)
    if case == 'two enter on one later frame':
        assert p.squeeze_idx == [0, 4, 12, 90] and p.first_frame.tolist() == [0, 2, 2] and p.new_frames == [2]
    if case == 'annotated frame with nothing new':
        assert p.new_frames == [2] and sorted(p.lut_new) == [2]
    if case == 'frame_index':
        assert p.first_frame.tolist() == [0, 5, 9] and p.new_frames == [5, 9]
    if case == 'void present':
        assert p.squeeze_idx == ([0, 1, 2] if void_label == 255 else [0, 1, 255, 2])
        assert p.lut_all[255] == (255 if void_label == 255 else 2) and p.lut_first[255] == (0 if void_label == 255 else 2)
    if case == '12 objects':
        assert p.num_objs == 12 and len(p.squeeze_idx) == 13


def test_protocol_refusals():
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.protocol import protocol_from_census
    labels = CASES['frame_index'][0]
    area = census_ref.census(labels)[:, :, 0]
    with pytest.raises(RmemError, match='start at 0'):
        protocol_from_census(area, [1, 5, 9])
    with pytest.raises(RmemError, match='increasing'):
        protocol_from_census(area, [0, 5, 5])
    with pytest.raises(RmemError, match='increasing'):
        protocol_from_census(area, [0, 9, 5])
    with pytest.raises(RmemError, match='entries'):
        protocol_from_census(area, [0, 5])
    empty_first = census_ref.census(_stack([[], [(3, 1, 1)]]))[:, :, 0]
    with pytest.raises(RmemError, match='no object on frame 0'):
        protocol_from_census(empty_first)
    void_first = census_ref.census(_stack([[(255, 0, 0)], [(3, 1, 1)]]))[:, :, 0]
    with pytest.raises(RmemError, match='no object on frame 0'):
        protocol_from_census(void_first)
    assert protocol_from_census(void_first, void_label=None).squeeze_idx == [0, 255, 3]


@pytest.mark.parametrize('case', sorted(CASES))
def test_squeeze_idx_round_trip(case):
    """what save_masks does with protocol.squeeze_idx undoes lut_all for every object id"""
    from rmem_ocu_amd import png
    from rmem_ocu_amd.protocol import protocol_from_census
    labels, frame_index = CASES[case]
    p = protocol_from_census(census_ref.census(labels)[:, :, 0], frame_index)
    back = png.squeeze_lut(p.squeeze_idx)
    assert p.num_objs >= 1
    for v in p.squeeze_idx[1:]:
        assert back[p.lut_all[v]] == v
    objects = np.isin(labels, p.squeeze_idx[1:])
    assert np.array_equal(back[p.lut_all[labels]][objects], labels[objects])


def test_summary_per_object():
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import summarize_scores, summarize_scores_per_object
    rng = np.random.default_rng(11)
    for n, objs in ((12, 1), (30, 3), (47, 5)):
        J, F = rng.random((n, objs)), rng.random((n, objs))
        for tail in (0.25, 0.5):
            a, b = summarize_scores_per_object(J, F, [0] * objs, tail), summarize_scores(J, F, tail=tail)
            for k, v in vars(b).items():
                if k == 'obj_frames':
                    continue
                assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(v)), (k, n, objs)
            assert b.obj_frames is None and all(np.array_equal(s, b.frames) for s in a.obj_frames)
            first = [int(t) for t in rng.integers(0, n - 3, objs)]
            first[0] = max(first[0], 1)                            # at least one object starts late
            census_ref.assert_score_equals(summarize_scores_per_object(J, F, first, tail), census_ref.per_object_summary(J, F, first, tail))
    J, F = rng.random((8, 2)), rng.random((8, 2))
    got = summarize_scores_per_object(J, F, [0, 5])                 # frames 6..6: one frame is enough
    assert got.obj_frames[1].tolist() == [6]
    with pytest.raises(RmemError, match='object 2'):
        summarize_scores_per_object(J, F, [0, 6])
    with pytest.raises(RmemError, match='first frames'):
        summarize_scores_per_object(J, F, [0])


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_entry_points_refuse_on_the_host(lib):
    """null pointer, n = 0, H * W > 2^26: non-zero, a message, nothing launched (there is no GPU in this tier)"""
    fake = 4096                                                     # a non-null address that is never dereferenced on the host
    for args, word in (((None, 1, 4, 4, fake, None), b'null'), ((fake, 1, 4, 4, None, None), b'null'),
                       ((fake, 0, 4, 4, fake, None), b'1..65535'), ((fake, 65536, 4, 4, fake, None), b'1..65535'),
                       ((fake, 1, 8193, 8193, fake, None), b'2^26'), ((fake, 1, 0, 4, fake, None), b'positive'),
                       ((fake, 1, 4, -1, fake, None), b'positive')):
        rc = lib.rmem_label_census(*args)
        assert rc != 0 and b'rmem_label_census' in lib.rmem_last_error_string() and word in lib.rmem_last_error_string(), args
    for args, word in (((None, fake, 1, 16, fake, 0, None), b'null'), ((fake, None, 1, 16, fake, 0, None), b'null'),
                       ((fake, fake, 1, 16, None, 0, None), b'null'), ((fake, fake, 0, 16, fake, 0, None), b'1..65535'),
                       ((fake, fake, 1, (1 << 26) + 1, fake, 1, None), b'2^26'), ((fake, fake, 1, 0, fake, 1, None), b'2^26')):
        rc = lib.rmem_label_remap(*args)
        assert rc != 0 and b'rmem_label_remap' in lib.rmem_last_error_string() and word in lib.rmem_last_error_string(), args


def test_host_tensors_are_refused():
    import torch
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.protocol import clip_protocol, label_census, remap_labels
    x = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for fn in (label_census, clip_protocol, lambda t: remap_labels(t, np.zeros(256, dtype=np.uint8))):
        with pytest.raises(RmemError, match='device tensor'):
            fn(x)
