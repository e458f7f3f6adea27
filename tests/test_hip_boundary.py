"""Clip scoring on the MI355X (rmem_clip_score_counts, evaluator.clip_counts / boundary_accuracy / score_clip): all six counts per
(frame, id) equal the numpy restatement of the DAVIS measures (tests/boundary_ref.py) exactly; the float scores built from them
agree to 1e-12."""
import numpy as np
import pytest
import torch

import boundary_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

# (H, W, ids incl. background): r = 8, 18, 2, 1, 1 (narrower than one word), 2 (width 1 modulo 64); 64 and 1920 are multiples of 64.
# 1080x1920 carries two objects only: the restatement needs seconds per object there.
SIZES = [(480, 854, 5), (1080, 1920, 3), (97, 131, 5), (64, 64, 5), (40, 50, 5), (33, 129, 5)]


def content_case(H, W, n_ids, kind):
    """annotation = seeded blobs; prediction = the annotation shifted and speckled, by less than r ('near'; by exactly
    one pixel where r = 1, still inside the disk, so that the match depends on the dilation) or by more ('far')"""
    r = R.radius(H, W)
    gt = R.blobs(H, W, n_ids, seed=H + W)
    dy, dx = (max(r // 2, 1), -(r // 2)) if kind == 'near' else (r + 3, -(r + 5))      # 'near' moves by at least one pixel, also at r = 1
    pred = R.shifted_speckled(gt, dy, dx, seed=H, speckles=max(40, H * W // 2000))
    return pred, gt


def device_counts(pred, gt, num_ids, **kw):
    from rmem_ocu_amd import evaluator
    c = evaluator.clip_counts(torch.from_numpy(np.ascontiguousarray(pred)).to(DEV), torch.from_numpy(np.ascontiguousarray(gt)).to(DEV),
                              num_ids, **kw)
    assert c.dtype == torch.int64 and c.is_cuda
    return c.cpu().numpy()


def check(pred, gt, num_ids, **kw):
    """device counts == restatement, for a frame [H, W] or a stack [n, H, W]; returns the reference counts [n, num_ids, 6]"""
    pred, gt = np.asarray(pred, dtype=np.uint8), np.asarray(gt, dtype=np.uint8)
    ref = R.clip_counts(pred[None], gt[None], num_ids, **kw) if pred.ndim == 2 else R.clip_counts(pred, gt, num_ids, **kw)
    got = device_counts(pred, gt, num_ids, **kw)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), f'first differing (frame, id, count): {np.argwhere(got != ref)[:5].tolist()}'
    return ref


@pytest.mark.parametrize('kind', ['near', 'far'])
@pytest.mark.parametrize('H,W,n_ids', SIZES)
def test_counts_equal_restatement(H, W, n_ids, kind):
    pred, gt = content_case(H, W, n_ids, kind)
    ref = R.frame_counts(pred, gt, n_ids)
    # the case must exercise the dilation: at least half of the scored ids partly matched, in the restatement's own output
    partly = [(0 < ref[k, 2] < ref[k, 0]) for k in range(1, n_ids)]
    print(f'{H}x{W} {kind}: r={R.radius(H, W)} fg_match/n_fg = {[(int(ref[k, 2]), int(ref[k, 0])) for k in range(1, n_ids)]}')
    assert 2 * sum(partly) >= len(partly), partly
    got = device_counts(pred, gt, n_ids)
    assert np.array_equal(got[0], ref), f'first differing (id, count): {np.argwhere(got[0] != ref)[:5].tolist()}'


def test_object_touching_all_borders():
    H, W = 70, 150
    gt = np.zeros((H, W), np.uint8)
    gt[:, 60:90] = 1
    gt[25:45, :] = 1                                  # a cross that reaches all four borders and both last row / last column
    gt[0:10, 0:10] = 2
    gt[H - 12:, W - 20:] = 3                          # covers the bottom-right pixel
    pred = R.shifted_speckled(gt, 2, 3, seed=1, speckles=10)
    ref = check(pred, gt, 4)
    assert (ref[0, 1:, 0] > 0).all() and (ref[0, 1:, 1] > 0).all()


def test_object_filling_the_frame():
    H, W = 48, 130
    full = np.ones((H, W), np.uint8)
    ref = check(full, full, 3)
    assert ref[0, 1].tolist() == [0, 0, 0, 0, H * W, H * W]          # a mask without a hole or an edge has no boundary pixel
    hole = full.copy()
    hole[20:24, 60:70] = 0
    check(hole, full, 3)
    check(full, hole, 3)


def test_ids_on_one_side_only_and_background_frame():
    H, W = 60, 100
    gt = np.zeros((3, H, W), np.uint8)
    pred = np.zeros((3, H, W), np.uint8)
    gt[0, 10:30, 10:40] = 1
    pred[0, 12:30, 10:42] = 1
    pred[0, 40:50, 60:90] = 2                          # only in the prediction
    gt[0, 35:55, 5:25] = 3                             # only in the annotation
    gt[2, 5:50, 5:90] = 2                              # frame 1 stays all background on both sides
    pred[2, 5:50, 5:90] = 2
    ref = check(pred, gt, 5)
    assert ref[0, 2, 0] > 0 and ref[0, 2, 1] == 0 and ref[0, 3, 0] == 0 and ref[0, 3, 1] > 0
    assert not ref[1].any() and not ref[:, 4].any()


def test_void_rectangle_cuts_an_object():
    H, W = 80, 140
    gt = R.blobs(H, W, 4, seed=3)
    pred = R.shifted_speckled(gt, 2, -1, seed=3, speckles=20)
    with_void = gt.copy()
    with_void[30:50, 40:100] = 255
    ref = check(pred, with_void, 4)
    assert not np.array_equal(ref, R.clip_counts(pred[None], gt[None], 4))       # the void region changes the counts
    check(pred, with_void, 4, void_label=7)                                        # another void label: 255 is then an ordinary id >= num_ids


def test_explicit_integer_radius():
    pred, gt = content_case(97, 131, 5, 'far')
    a = check(pred, gt, 5, bound_th=3)
    b = check(pred, gt, 5, bound_th=11)
    assert (b[0, 1:, 2] >= a[0, 1:, 2]).all() and (b[0, 1:, 2] > a[0, 1:, 2]).any()
    gt2 = R.blobs(90, 300, 5, seed=9)
    check(R.shifted_speckled(gt2, 30, -50, seed=9), gt2, 5, bound_th=63)           # the largest radius: 63 bits of a neighbouring word


def test_radius_beyond_one_word_is_refused():
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    x = torch.zeros(40, 50, dtype=torch.uint8, device=DEV)
    with pytest.raises(RmemError, match='radius'):
        evaluator.clip_counts(x, x, 3, bound_th=64)


def batch6():
    H, W = 97, 131
    gts = np.stack([R.blobs(H, W, 5, seed=20 + i) for i in range(6)])
    preds = np.stack([R.shifted_speckled(gts[i], 1 + i, 2 - i, seed=30 + i) for i in range(6)])
    preds[4] = 0                                       # nothing predicted
    gts[5, 40:60, 30:80] = 255
    return preds, gts


def test_batch_equals_single_frames_and_restatement():
    preds, gts = batch6()
    ref = check(preds, gts, 5)
    for i in range(6):
        assert np.array_equal(device_counts(preds[i], gts[i], 5)[0], ref[i])


def test_j_counts_equal_mask_iou_counts():
    from rmem_ocu_amd import _lib
    preds, gts = batch6()
    got = device_counts(preds, gts, 5)
    for i in range(6):
        p, g = torch.from_numpy(preds[i]).to(DEV), torch.from_numpy(gts[i]).to(DEV)
        c = torch.zeros(10, dtype=torch.int64, device=DEV)
        _lib.check(_lib.lib().rmem_mask_iou_counts(p.data_ptr(), g.data_ptr(), p.numel(), 5, 255, c.data_ptr(),
                                                   torch.cuda.current_stream(DEV).cuda_stream), 'rmem_mask_iou_counts')
        assert np.array_equal(got[i, :, 4:6], c.cpu().numpy().reshape(5, 2))


def test_same_workspace_twice():
    """the counts are re-zeroed and every plane rewritten: A, then other frames of the same size, then A again"""
    preds, gts = batch6()
    a = device_counts(preds, gts, 5)
    assert np.array_equal(device_counts(preds, gts, 5), a)
    other = device_counts(gts[::-1].copy(), preds[::-1].copy(), 5)
    assert not np.array_equal(other, a)
    assert np.array_equal(device_counts(preds, gts, 5), a)


def test_boundary_accuracy_end_to_end():
    from rmem_ocu_amd import evaluator
    pred, gt = content_case(97, 131, 5, 'far')
    pred[pred == 4] = 0
    gt[gt == 4] = 0                                    # id 4 absent from both masks: skipped
    pred[0:3, 0:3] = 6                                 # only predicted
    got = evaluator.boundary_accuracy(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    ref = R.frame_counts(pred, gt, 11)
    want = {k: R.f_from_counts(*[int(v) for v in ref[k, :4]]) for k in range(1, 11) if ref[k, 5] > 0}
    assert sorted(got) == sorted(want) == [1, 2, 3, 6]
    assert all(abs(got[k] - want[k]) < 1e-12 for k in want)
    assert got[6] == 0.0 and got[1] == 0.0 and 0.0 < got[2] < 1.0      # id 1 moved out of reach of its annotation: nothing matched
    j = evaluator.region_similarity(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    assert sorted(j) == sorted(got)


def test_score_clip_end_to_end():
    from rmem_ocu_amd import evaluator
    H, W, n = 64, 96, 9
    base = R.blobs(H, W, 4, seed=5)
    gts = np.stack([R.shifted_speckled(base, i, i // 2, seed=50, speckles=0) for i in range(n)])
    gts[6:][gts[6:] == 2] = 0                          # object 2 vanishes from frame 6 on
    preds = np.stack([R.shifted_speckled(gts[i], i // 2, -(i // 3), seed=60 + i, speckles=5 * i) for i in range(n)])
    preds[7][preds[7] == 2] = 0                        # empty against empty on frame 7; frame 8 may carry speckles of id 2
    gts[3, 20:30, 40:60] = 255
    p, g = torch.from_numpy(preds).to(DEV), torch.from_numpy(gts).to(DEV)
    for kw in (dict(), dict(num_objs=3), dict(num_objs=2, frames=slice(0, None), tail=0.5), dict(frames=[1, 2, 5, 6, 7])):
        got = evaluator.score_clip(p, g, **kw)
        nobj = kw.get('num_objs', 3)
        Jr, Fr = R.scores(R.clip_counts(preds, gts, nobj + 1))
        Jr, Fr = Jr[:, 1:], Fr[:, 1:]
        assert got.J.shape == (n, nobj) and np.abs(got.J - Jr).max() < 1e-12 and np.abs(got.F - Fr).max() < 1e-12
        want = R.summary(Jr, Fr, kw.get('frames', slice(1, -1)), kw.get('tail', 0.25))
        for name, v in want.items():
            assert np.abs(np.asarray(getattr(got, name)) - np.asarray(v)).max() < 1e-12, name
    assert got.J[7, 1] == 1.0 and got.F[7, 1] == 1.0   # empty against empty scores 1


def test_bad_inputs_raise_with_a_message():
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    a = torch.zeros(2, 40, 50, dtype=torch.uint8, device=DEV)
    with pytest.raises(RmemError, match='shape'):
        evaluator.clip_counts(a, a[:, :, :49])
    with pytest.raises(RmemError, match='uint8'):
        evaluator.clip_counts(a.float(), a.float())
    with pytest.raises(RmemError, match='device'):
        evaluator.clip_counts(a.cpu(), a.cpu())
    with pytest.raises(RmemError, match='num_ids'):
        evaluator.clip_counts(a, a, num_ids=33)
    with pytest.raises(RmemError, match='no frame'):
        evaluator.score_clip(a, a, num_objs=1)          # two frames: the default selection drops both
