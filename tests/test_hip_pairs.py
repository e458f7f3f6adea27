"""The pair census on the MI355X against tests/pair_ref.py: exact integer equality everywhere.  Both stacks sit between guard
bytes and start at any byte independently, the output is dirtied first and followed by guard ints, both routes (table in LDS,
table in global memory) are crossed at the constant the library reports.  Then what is built on the table: the marginals against
protocol.label_census, the diagonal against evaluator.clip_counts, relabel_to_match, identity_report and the run-length plumbing."""
import functools
import math

import numpy as np
import pytest
import torch

import census_ref
import pair_ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
SMALL = [(1, 1, 1), (1, 1, 17), (2, 3, 5), (3, 17, 33), (2, 37, 131), (4, 64, 256)]
FULL = (1, 480, 854)
CONTENTS = ['zero', 'identical', 'shifted', 'noise', 'stripes', 'void', 'above']
OFFSETS = [(0, 0), (1, 1), (3, 13), (13, 0), (0, 7)]


def _sid(s):
    return 'x'.join(map(str, s))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _lds_bins():
    from rmem_ocu_amd import _lib
    return int(_lib.lib().rmem_label_pair_census_lds_bins())


def _nums():
    """(num_a, num_b): both routes, and both sides of the LDS constant"""
    bins = _lds_bins()
    k = math.isqrt(bins) - 2                                       # the largest square that fits: (k + 2)^2 <= bins
    over = (k + 1, k) if (k + 3) * (k + 2) > bins else (k + 1, k + 1)   # the smallest pair that does not
    assert (k + 2) ** 2 <= bins < (over[0] + 2) * (over[1] + 2)
    return [(1, 1), (10, 10), (31, 5), (k, k), over, (255, 255)]


@functools.lru_cache(maxsize=None)
def _content(shape, content, num_a, num_b):
    """(a, b) of one (shape, content) for tables of (num_a, num_b): computed once, shared, read only"""
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W + 17 * num_a + num_b)
    ids = tuple(range(1, min(num_a, num_b, 10) + 1))
    blobs = census_ref.blobs(H * W + n, n, H, W, ids=ids)
    if content == 'zero':
        a, b = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    elif content == 'identical':
        a, b = blobs, blobs.copy()
    elif content == 'shifted':
        a, b = blobs, np.roll(blobs, (2, 3), axis=(1, 2))
    elif content == 'noise':                                       # num + 1 ids each: every lane mixed, every wave holds every pair
        a = rng.integers(0, min(num_a + 1, 255) + 1, shape).astype(np.uint8)
        b = rng.integers(0, min(num_b + 1, 255) + 1, shape).astype(np.uint8)
    elif content == 'stripes':                                     # a constant, b vertical one-pixel stripes: lanes mixed in one stack only
        a = np.full(shape, min(num_a, 3), dtype=np.uint8)
        b = np.zeros(shape, dtype=np.uint8)
        b[:] = (np.arange(W) % 3).astype(np.uint8)[None, None, :]
    elif content == 'void':                                        # 10 % of b is 255
        a, b = blobs, np.roll(blobs, (1, 2), axis=(1, 2))
        b[rng.random(shape) < 0.1] = 255
    else:                                                          # 'above': a holds values past num_a, 255 among them
        a, b = blobs.copy(), np.roll(blobs, (2, 3), axis=(1, 2))
        hit = rng.random(shape) < 0.2
        a[hit] = rng.integers(min(num_a + 1, 255), 256, shape).astype(np.uint8)[hit]
    for t in (a, b):
        t.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(shape, content, num_a, num_b):
    a, b = _content(shape, content, num_a, num_b)
    want = pair_ref.census(a, b, num_a, num_b)
    want.setflags(write=False)
    return want


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _guards_intact(buf, front, size):
    h = buf.cpu().numpy()
    return (h[:front] == CANARY).all() and (h[front + size:] == CANARY).all()


def _pairs(dev, a, b, num_a, num_b, offsets=(0, 0)):
    """rmem_label_pair_census on guarded copies of a and b, out pre-filled with 0xA5 and followed by guard ints"""
    from rmem_ocu_amd import _lib
    n, H, W = a.shape
    abuf, aview, afront = _guarded(dev, a, offsets[0])
    bbuf, bview, bfront = _guarded(dev, b, offsets[1])
    size = n * (num_a + 2) * (num_b + 2)
    out = torch.full((size + 64,), CANARY32, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().rmem_label_pair_census(aview.data_ptr(), bview.data_ptr(), n, H, W, num_a, num_b, out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), 'rmem_label_pair_census')
    torch.cuda.synchronize()
    assert _guards_intact(abuf, afront, a.size) and _guards_intact(bbuf, bfront, b.size), 'guard bytes around the stacks'
    assert np.array_equal(abuf[afront:afront + a.size].cpu().numpy(), a.reshape(-1)), 'a is read only'
    assert np.array_equal(bbuf[bfront:bfront + b.size].cpu().numpy(), b.reshape(-1)), 'b is read only'
    o = out.cpu().numpy()
    assert (o[size:] == CANARY32).all(), 'ints beyond the table were written'
    return o[:size].reshape(n, num_a + 2, num_b + 2)


def _check(dev, shape, content, num_a, num_b, offsets=(0, 0)):
    a, b = _content(shape, content, num_a, num_b)
    got, want = _pairs(dev, a, b, num_a, num_b, offsets), _ref(shape, content, num_a, num_b)
    assert np.array_equal(got, want), (content, num_a, num_b, offsets, np.argwhere(got != want)[:8])
    assert (got.astype(np.int64).sum(axis=(1, 2)) == shape[1] * shape[2]).all()


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SMALL, ids=_sid)
def test_pair_census_contents(dev, shape, content):
    """every content at every small shape, one table in LDS and one in global memory"""
    _check(dev, shape, content, 10, 10)
    _check(dev, shape, content, 255, 255)


@pytest.mark.parametrize('k', range(6), ids=['1x1', '10x10', '31x5', 'largest in LDS', 'smallest beyond', '255x255'])
def test_pair_census_table_sizes(dev, k):
    num_a, num_b = _nums()[k]
    for shape in ((3, 17, 33), (4, 64, 256)):
        for content in ('shifted', 'noise', 'void', 'above'):
            _check(dev, shape, content, num_a, num_b, (3, 13))


@pytest.mark.parametrize('offsets', OFFSETS, ids=lambda o: f'{o[0]}+{o[1]}')
@pytest.mark.parametrize('shape', SMALL, ids=_sid)
def test_pair_census_byte_offsets(dev, shape, offsets):
    """the two stacks start at any byte, independently: both routes, and a noise content for the per-lane masks"""
    _check(dev, shape, 'shifted', 10, 10, offsets)
    _check(dev, shape, 'noise', 10, 10, offsets)
    _check(dev, shape, 'shifted', 255, 255, offsets)


@pytest.mark.parametrize('num', [10, 255], ids=['LDS', 'global'])
def test_pair_census_full_size_frame(dev, num):
    """one 480 x 854 frame per route, at every offset pair"""
    for offsets in OFFSETS:
        _check(dev, FULL, 'void', num, num, offsets)
    _check(dev, FULL, 'noise', num, num, (3, 13))


# ------------------------------------------------------------------------------------------------------------------ yardsticks
def test_marginals_equal_the_label_census(dev):
    """row sums = areas of a, column sums = areas of b, for every value up to num (protocol.label_census, another kernel)"""
    from rmem_ocu_amd.pairs import pair_census
    from rmem_ocu_amd.protocol import label_census
    for shape, num_a, num_b in (((3, 17, 33), 10, 10), ((4, 64, 256), 31, 5), ((2, 37, 131), 255, 255)):
        for content in ('void', 'above', 'noise'):
            a, b = (torch.from_numpy(t.copy()).to(dev) for t in _content(shape, content, num_a, num_b))
            C = pair_census(a, b, num_a, num_b)
            assert C.dtype == torch.int32 and tuple(C.shape) == (shape[0], num_a + 2, num_b + 2)
            C = C.cpu().numpy().astype(np.int64)
            area_a, area_b = label_census(a)[0].cpu().numpy(), label_census(b)[0].cpu().numpy()
            assert np.array_equal(C.sum(axis=2)[:, :num_a + 1], area_a[:, :num_a + 1])
            assert np.array_equal(C.sum(axis=1)[:, :num_b + 1], area_b[:, :num_b + 1])
            assert np.array_equal(C.sum(axis=2)[:, num_a + 1], area_a[:, num_a + 1:].sum(axis=1))
            assert np.array_equal(C.sum(axis=1)[:, num_b + 1], area_b[:, num_b + 1:].sum(axis=1))
    one = pair_census(a[0], b[0], 255, 255)                        # [H, W] is one frame
    assert tuple(one.shape) == (1, 257, 257) and np.array_equal(one.cpu().numpy()[0], C[0])


def test_diagonal_equals_clip_counts(dev):
    """with void in b, intersection and union on the diagonal after drop_other_b are rmem_clip_score_counts' J counts"""
    from rmem_ocu_amd.evaluator import clip_counts
    from rmem_ocu_amd.pairs import pair_census, pair_iou
    for shape, num in (((3, 17, 33), 10), ((4, 64, 256), 5), ((2, 37, 131), 31)):
        a, b = _content(shape, 'void', num, num)
        assert (b == 255).any()
        ad, bd = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
        iou, inter, union = pair_iou(pair_census(ad, bd, num, num), drop_other_b=True)
        counts = clip_counts(ad, bd, num + 1, 255).cpu().numpy()
        d = np.arange(num)
        assert np.array_equal(inter[:, d, d], counts[:, 1:, 4]) and np.array_equal(union[:, d, d], counts[:, 1:, 5])
        w_iou, w_inter, w_union = pair_ref.pair_iou(a, b, num, num, True)
        assert np.array_equal(inter, w_inter) and np.array_equal(union, w_union) and np.array_equal(iou, w_iou, equal_nan=True)


def test_side_stream_twice(dev):
    """on a non-default stream, after the output was dirtied there, twice in a row: identical bytes, and the reference's"""
    from rmem_ocu_amd.pairs import pair_census
    side = torch.cuda.Stream(dev)
    for num in (10, 255):
        shape = (4, 64, 256)
        a, b = (torch.from_numpy(t.copy()).to(dev) for t in _content(shape, 'noise', num, num))
        side.wait_stream(torch.cuda.current_stream(dev))
        got = []
        with torch.cuda.stream(side):
            for _ in range(2):
                torch.full((shape[0] * (num + 2) * (num + 2),), CANARY32, dtype=torch.int32, device=dev)   # the block the table gets next
                got.append(pair_census(a, b, num, num))
            side.synchronize()
        assert torch.equal(got[0], got[1]) and np.array_equal(got[0].cpu().numpy(), _ref(shape, 'noise', num, num))
        assert got[0].cpu().numpy().tobytes() == got[1].cpu().numpy().tobytes()


def test_python_refusals_on_the_device(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.pairs import pair_census
    x = torch.zeros(2, 4, 4, dtype=torch.uint8, device=dev)
    with pytest.raises(RmemError, match='one shape'):
        pair_census(x, x[:1], 3, 3)
    with pytest.raises(RmemError, match='one shape'):
        pair_census(x[0], x[:1], 3, 3)
    with pytest.raises(RmemError, match='device tensor'):
        pair_census(x, x.cpu(), 3, 3)
    with pytest.raises(RmemError, match='device tensor'):
        pair_census(x, x.int(), 3, 3)
    with pytest.raises(RmemError, match='num_b'):
        pair_census(x, x, 3, 256)


# ------------------------------------------------------------------------------------------------------------ the evaluator
def _clip(n=6, H=48, W=80, num=4, void=True):
    """annotations with `num` objects that drift, and a prediction: the annotation moved by (1, 2) pixels, void cleared"""
    gt = np.zeros((n, H, W), dtype=np.uint8)
    for v in range(1, num + 1):                                     # boxes of (6 + 2 v) x (8 + 3 v) side by side, one pixel down per frame
        x = 2 + 18 * (v - 1)
        for f in range(n):
            gt[f, 3 + v + f:9 + 3 * v + f, x:x + 8 + 3 * v] = v
    pred = np.roll(gt, (1, 2), axis=(1, 2))
    if void:
        gt[:, 0, W - 9:] = 255
    return pred, gt


def test_relabel_to_match(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import relabel_to_match, score_clip
    pred, gt = _clip()
    assert all((pred == v).any() and (gt == v).any() for v in (1, 2, 3, 4))
    perm = np.arange(256, dtype=np.uint8)
    perm[[1, 2, 3, 4]] = [3, 1, 4, 2]                               # the run's id of the annotation's 1 is 3, ...
    pred_d, gt_d, mixed_d = (torch.from_numpy(t).to(dev) for t in (pred, gt, perm[pred]))
    back, mapping, iou = relabel_to_match(mixed_d, gt_d, 4, 4)
    assert mapping == {3: 1, 1: 2, 4: 3, 2: 4} and back.dtype == torch.uint8 and torch.equal(back, pred_d)
    assert iou.shape == (4, 4) and np.array_equal(iou, pair_ref.track_iou(perm[pred], gt, 4, 4))
    got, want = score_clip(back, gt_d, 4), score_clip(pred_d, gt_d, 4)
    for k, v in vars(want).items():
        if k != 'obj_frames':
            assert np.array_equal(np.asarray(getattr(got, k)), np.asarray(v)), k
    # an extra predicted object that lies on nothing annotated gets num_gt + 1, the matched ones keep their partners
    extra = perm[pred].copy()
    free = np.argwhere((gt == 0).all(axis=0) & (pred == 0).all(axis=0))[0]
    extra[:, free[0], free[1]] = 5
    back, mapping, iou = relabel_to_match(torch.from_numpy(extra).to(dev), gt_d, 5, 4)
    assert mapping == {1: 2, 2: 4, 3: 1, 4: 3, 5: 5} and (iou[4] == 0).all()
    want = pred.copy()
    want[:, free[0], free[1]] = 5
    assert np.array_equal(back.cpu().numpy(), want)
    with pytest.raises(RmemError, match='255'):                     # 254 annotated ids, two predicted ids without a partner
        relabel_to_match(torch.from_numpy(extra).to(dev), torch.zeros_like(gt_d), 5, 254)


def _swap_clip():
    """[6, 40, 64]: annotated objects 1 and 2 stand still; the prediction follows them on frames 0..2 and trades them from 3 on"""
    gt = np.zeros((6, 40, 64), dtype=np.uint8)
    gt[:, 4:16, 6:26] = 1
    gt[:, 22:36, 34:58] = 2
    gt[:, 39, 60:] = 255
    pred = np.where(gt == 255, 0, gt).astype(np.uint8)
    swapped = pred.copy()
    swapped[3:][pred[3:] == 1] = 2
    swapped[3:][pred[3:] == 2] = 1
    return pred, swapped, gt


def test_identity_report(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import identity_report, score_clip
    clean, swapped, gt = _swap_clip()
    gt_d = torch.from_numpy(gt).to(dev)
    rep = identity_report(torch.from_numpy(swapped).to(dev), gt_d, 2)
    assert sorted(rep) == [1, 2]
    a1, a2 = 12 * 20, 14 * 24                                       # three frames apart, three frames on the other's place
    assert rep[1].rival == 2 and rep[2].rival == 1 and rep[1].rival_iou == a2 / (a1 + 2 * a2) and rep[2].rival_iou == a1 / (2 * a1 + a2)
    assert rep[1].switch_frames == [3, 4, 5] and rep[2].switch_frames == [3, 4, 5]
    assert rep[1].J_own.tolist() == [1, 1, 1, 0, 0, 0] and rep[2].J_own.tolist() == [1, 1, 1, 0, 0, 0]
    rep = identity_report(torch.from_numpy(clean).to(dev), gt_d, 2)
    for i in (1, 2):
        assert rep[i].rival is None and rep[i].rival_iou == 0.0 and rep[i].switch_frames == [] and rep[i].J_own.tolist() == [1] * 6
    # 40 objects, where score_clip refuses: boxes of 4 x 6 on a grid, the prediction one pixel to the right; 7 and 8 trade on frame 1
    gt = np.zeros((2, 40, 64), dtype=np.uint8)
    for k in range(40):
        y, x = 5 * (k // 8), 8 * (k % 8)
        gt[:, y:y + 4, x:x + 6] = k + 1
    pred = np.roll(gt, 1, axis=2)
    pred[1][np.roll(gt[1], 1, axis=1) == 7], pred[1][np.roll(gt[1], 1, axis=1) == 8] = 8, 7
    pred_d, gt_d = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    with pytest.raises(RmemError, match='1..31'):
        score_clip(pred_d, gt_d, 40)
    rep = identity_report(pred_d, gt_d, 40)
    assert sorted(rep) == list(range(1, 41))
    iou, inter, union = pair_ref.pair_iou(pred, gt, 40, 40)
    for i in range(1, 41):
        assert np.array_equal(rep[i].J_own, iou[:, i - 1, i - 1])
        assert rep[i].switch_frames == ([1] if i in (7, 8) else [])
    assert rep[7].rival == 8 and rep[8].rival == 7 and rep[7].rival_iou == rep[8].rival_iou == 20 / 76
    assert all(rep[i].rival is None and rep[i].rival_iou == 0.0 for i in range(1, 41) if i not in (7, 8))   # a box moved by one pixel touches its own only
    with pytest.raises(RmemError, match='void_label'):
        identity_report(pred_d, gt_d, 40, void_label=40)


def test_run_length_plumbing(dev):
    """two tracks delivered as run-length strings against the same annotations delivered as palette PNGs: track IoU exactly 1 on
    the matched pairs and 0 elsewhere, and relabel_to_match finds the pairs"""
    import rle_ref
    from rmem_ocu_amd import png
    from rmem_ocu_amd.evaluator import labels_from_pngs, labels_from_rles, relabel_to_match, score_clip
    from rmem_ocu_amd.pairs import pair_census, track_iou
    a = np.zeros((4, 37, 131), dtype=np.uint8)
    for f in range(4):
        a[f, 2 + f:12 + f, 5:40] = 7
        a[f, 20:30, 60 + 3 * f:100 + 3 * f] = 3
    tracks = [{('car' if v == 7 else 'bike'): {'size': [37, 131], 'counts': rle_ref.to_string(rle_ref.counts_of(fr == v)).decode()}
               for v in (3, 7)} for fr in a]
    from_rle, ids = labels_from_rles(tracks, (37, 131), dev)
    assert ids == ['bike', 'car']                                   # label values 1, 2
    from_png = labels_from_pngs(png.encode_label_stack(torch.from_numpy(a).to(dev)), dev)     # original ids 3, 7
    iou = track_iou(pair_census(from_rle, from_png, 2, 7))
    want = np.zeros((2, 7))
    want[0, 2] = want[1, 6] = 1.0
    assert np.array_equal(iou, want)
    back, mapping, _ = relabel_to_match(from_rle, from_png, 2, 7)
    assert mapping == {1: 3, 2: 7} and torch.equal(back, from_png)
    # the README's chain the other way round: annotations from strings, predictions in other ids, scored in the annotation's
    pred, mapping, _ = relabel_to_match(from_png, from_rle, 7, 2)
    score = score_clip(pred, from_rle, 2)
    assert mapping[3] == 1 and mapping[7] == 2 and torch.equal(pred, from_rle) and score.J_mean == 1.0 and score.F_mean == 1.0
