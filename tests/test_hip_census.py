"""Label census, label remap and the clip protocol on the MI355X against tests/census_ref.py: exact integer / byte equality
everywhere.  Shapes: H * W and W odd, frames that start at any byte, rows shorter than one 16-byte load, one full-size frame."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import census_ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
SHAPES = [(1, 1, 1), (1, 1, 17), (3, 5, 33), (2, 37, 131), (4, 64, 256), (1, 480, 854)]
CONTENTS = ['zero', 'all 255', 'random', 'blobs', 'corners', 'stripes']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _stacks(shape, content):
    """the label stacks of one (shape, content): computed once, shared, read only"""
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    if content == 'zero':
        out = [np.zeros(shape, dtype=np.uint8)]
    elif content == 'all 255':
        out = [np.full(shape, 255, dtype=np.uint8)]
    elif content == 'random':
        out = [rng.integers(0, 256, shape).astype(np.uint8)]
    elif content == 'blobs':
        out = [census_ref.blobs(H * W + n, n, H, W)]
    elif content == 'corners':
        out = []
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            a = np.zeros(shape, dtype=np.uint8)
            a[:, y, x] = 7
            out.append(a)
    else:                                                          # vertical stripes one pixel wide: every lane's 16 bytes are mixed
        a = np.zeros(shape, dtype=np.uint8)
        a[:] = (np.arange(W) % 3 + 1).astype(np.uint8)[None, None, :]
        out = [a]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _census_ref(shape, content):
    return tuple(census_ref.census(a) for a in _stacks(shape, content))


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _guards_intact(buf, front, size):
    b = buf.cpu().numpy()
    return (b[:front] == CANARY).all() and (b[front + size:] == CANARY).all()


def _census(dev, a, offset=0):
    """rmem_label_census on a guarded copy of a, out pre-filled with 0xA5 and followed by guard ints"""
    from rmem_ocu_amd import _lib
    n, H, W = a.shape
    buf, view, front = _guarded(dev, a, offset)
    out = torch.full((n * 256 * 5 + 64,), CANARY32, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().rmem_label_census(view.data_ptr(), n, H, W, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               'rmem_label_census')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, a.size), 'guard bytes around the labels'
    assert np.array_equal(buf[front:front + a.size].cpu().numpy(), a.reshape(-1)), 'the labels are read only'
    o = out.cpu().numpy()
    assert (o[n * 256 * 5:] == CANARY32).all(), 'ints beyond n * 256 * 5 were written'
    return o[:n * 256 * 5].reshape(n, 256, 5)


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_census(dev, shape, content):
    for a, want in zip(_stacks(shape, content), _census_ref(shape, content)):
        got = _census(dev, a)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_census_unaligned_base(dev, shape, content, offset):
    for a, want in zip(_stacks(shape, content), _census_ref(shape, content)):
        got = _census(dev, a, offset)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_label_census_is_reproducible(dev):
    from rmem_ocu_amd.protocol import label_census
    for shape in ((4, 64, 256), (1, 480, 854)):
        for content in ('random', 'blobs'):
            t = torch.from_numpy(_stacks(shape, content)[0].copy()).to(dev)
            a1, b1 = label_census(t)
            a2, b2 = label_census(t)
            torch.cuda.synchronize()
            assert torch.equal(a1, a2) and torch.equal(b1, b2)
            want = _census_ref(shape, content)[0]
            assert a1.dtype == torch.int32 and tuple(a1.shape) == (shape[0], 256) and tuple(b1.shape) == (shape[0], 256, 4)
            assert np.array_equal(a1.cpu().numpy(), want[:, :, 0]) and np.array_equal(b1.cpu().numpy(), want[:, :, 1:])


def _luts(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 256)).astype(np.uint8)


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_remap(dev, shape, offset):
    """one table and one per frame, in place and out of place (dst at the source's alignment and at another one), guards intact"""
    from rmem_ocu_amd import _lib
    n, H, W = shape
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    for content in ('random', 'blobs', 'stripes', 'all 255'):
        a = _stacks(shape, content)[0]
        for per_frame in (0, 1):
            luts = _luts(n if per_frame else 1, H * W + per_frame)
            want = np.stack([luts[f if per_frame else 0][a[f]] for f in range(n)])
            luts_d = torch.from_numpy(luts).to(dev)
            for dst_offset in (None, offset, (offset + 5) % 16):   # None: in place
                sbuf, sview, sfront = _guarded(dev, a, offset)
                if dst_offset is None:
                    dbuf, dview, dfront = sbuf, sview, sfront
                else:
                    dbuf, dview, dfront = _guarded(dev, np.full(shape, 0x5A, dtype=np.uint8), dst_offset)
                _lib.check(L.rmem_label_remap(sview.data_ptr(), dview.data_ptr(), n, H * W, luts_d.data_ptr(), per_frame, s),
                           'rmem_label_remap')
                torch.cuda.synchronize()
                assert _guards_intact(dbuf, dfront, a.size) and _guards_intact(sbuf, sfront, a.size), (content, per_frame, dst_offset)
                got = dbuf[dfront:dfront + a.size].cpu().numpy().reshape(shape)
                assert np.array_equal(got, want), (content, per_frame, dst_offset)
                if dst_offset is not None:
                    assert np.array_equal(sbuf[sfront:sfront + a.size].cpu().numpy(), a.reshape(-1)), 'the source is read only'


def test_remap_labels_wrapper(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.protocol import remap_labels
    a = _stacks((3, 5, 33), 'random')[0]
    t = torch.from_numpy(a.copy()).to(dev)
    luts = _luts(3, 5)
    assert np.array_equal(remap_labels(t, luts[0]).cpu().numpy(), luts[0][a])
    assert np.array_equal(remap_labels(t, torch.from_numpy(luts).to(dev)).cpu().numpy(), np.stack([luts[f][a[f]] for f in range(3)]))
    assert np.array_equal(remap_labels(t[1], luts[1]).cpu().numpy(), luts[1][a[1]])
    assert remap_labels(t, luts[2], out=t) is t and np.array_equal(t.cpu().numpy(), luts[2][a])
    with pytest.raises(RmemError, match='luts'):
        remap_labels(t, luts[:2])
    with pytest.raises(RmemError, match='luts'):
        remap_labels(t, luts.astype(np.int32))


def _annotations():
    """[6, 37, 131]: ids 3 and 7 on frame 0, 200 enters on frame 4 (and 7 is hidden on frame 2); void pixels on every frame"""
    a = np.zeros((6, 37, 131), dtype=np.uint8)
    for f in range(6):
        a[f, 2 + f:12 + f, 5:40] = 7
        a[f, 20:30, 60 + 3 * f:100 + 3 * f] = 3
        a[f, 0, 120:131] = 255
    a[2][a[2] == 7] = 0
    for f in (4, 5):
        a[f, 8:19, 90 + f:117 + f] = 200
    return a


def test_clip_protocol(dev):
    from rmem_ocu_amd.protocol import clip_protocol
    a = _annotations()
    for rows, frame_index in ((list(range(6)), None), ([0, 2, 4], [0, 2, 4]), ([0, 3], [0, 3])):
        sub = a[rows]
        proto, first, new = clip_protocol(torch.from_numpy(sub.copy()).to(dev), frame_index)
        squeeze_idx, first_frame, new_frames = census_ref.protocol(sub, frame_index)
        assert proto.squeeze_idx == squeeze_idx and proto.first_frame.tolist() == first_frame and proto.new_frames == new_frames
        want_first, want_new = census_ref.overlays(sub, frame_index)
        assert first.dtype == torch.uint8 and np.array_equal(first.cpu().numpy(), want_first)
        assert sorted(new) == sorted(want_new)
        for t in want_new:
            assert np.array_equal(new[t].cpu().numpy(), want_new[t]), t
    assert squeeze_idx == [0, 3, 7] and not new                      # frames 0 and 3: nothing enters
    proto, first, new = clip_protocol(torch.from_numpy(a).to(dev))
    assert proto.squeeze_idx == [0, 3, 7, 200] and proto.first_frame.tolist() == [0, 0, 4] and sorted(new) == [4]
    assert set(np.unique(new[4].cpu().numpy())) == {0, 3}, 'an overlay holds the new objects only'


def test_object_boxes(dev):
    from rmem_ocu_amd.evaluator import object_boxes
    a = census_ref.blobs(5, 4, 64, 96, ids=(1, 2, 3, 4, 5, 9))
    a[2][a[2] == 3] = 0                                             # object 3 is absent from frame 2
    area, box = object_boxes(torch.from_numpy(a).to(dev), 6)
    want = census_ref.census(a)
    assert tuple(area.shape) == (4, 6) and tuple(box.shape) == (4, 6, 4)
    assert np.array_equal(area.cpu().numpy(), want[:, 1:7, 0]) and np.array_equal(box.cpu().numpy(), want[:, 1:7, 1:])
    assert area[2, 2].item() == 0 and box[2, 2].tolist() == [96, 64, -1, -1] and area[0, 5].item() == 0


def test_score_annotated_clip(dev):
    """[8, 64, 96], ids 3 and 7 from frame 0, 200 from frame 3: every summary field equals census_ref's per-object summary of
    clip_counts's own counts"""
    from rmem_ocu_amd.evaluator import clip_counts, score_annotated_clip, scores_from_counts
    from rmem_ocu_amd.protocol import clip_protocol
    gt = np.zeros((8, 64, 96), dtype=np.uint8)
    for f in range(8):
        gt[f, 4 + f:24 + f, 6:40] = 7
        gt[f, 30:50, 50 + 2 * f:80 + 2 * f] = 3
        gt[f, 63, 90:] = 255
        if f >= 3:
            gt[f, 5:20, 55 + f:75 + f] = 200
    gt_d = torch.from_numpy(gt).to(dev)
    proto = clip_protocol(gt_d)[0]
    assert proto.squeeze_idx == [0, 3, 7, 200] and proto.first_frame.tolist() == [0, 0, 3]
    pred = proto.lut_all[gt]
    pred[pred == 255] = 0
    pred = np.roll(pred, (1, 2), axis=(1, 2))                       # an imperfect prediction in squeezed ids
    pred[:3][pred[:3] == 3] = 0
    pred_d = torch.from_numpy(pred).to(dev)
    score = score_annotated_clip(pred_d, gt_d, proto)
    counts = clip_counts(pred_d, torch.from_numpy(proto.lut_all[gt]).to(dev), 4).cpu().numpy()
    J, Fm = scores_from_counts(counts)
    census_ref.assert_score_equals(score, census_ref.per_object_summary(J[:, 1:], Fm[:, 1:], [0, 0, 3]))
    assert np.array_equal(score.J, J[:, 1:]) and np.array_equal(score.F, Fm[:, 1:])
    assert [s.tolist() for s in score.obj_frames] == [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [4, 5, 6]]
    assert 0.0 < score.J_obj_mean[2] < 1.0


def test_run_annotated_clips(dev, tmp_path):
    """The ragged geometry (make_clip(..., 161, 193, 2), output 160 x 192, bank 1 + 7, rows 2, lookahead 2), clips of 9 and 14
    frames annotated in sparse ids 4 and 9; in the longer one id 6 enters at frame 6.  The stacks equal run_clips's when it is
    given the first label and the overlay built by hand on the host, and the written files read back in the sparse ids."""
    from rmem_ocu_amd import png
    from rmem_ocu_amd.evaluator import labels_from_pngs, run_annotated_clips, run_clips, save_masks
    from test_hip_ragged_group import NET, OUT, _clip, _model
    sparse = np.zeros(256, dtype=np.uint8)
    sparse[1], sparse[2] = 4, 9
    clips, by_hand, anns = [], [], {}
    for cid, n in (('short', 9), ('long', 14)):
        f, m = _clip(n)
        small = F.interpolate(m.float(), size=OUT, mode='nearest')[0, 0].numpy().astype(np.uint8)     # ids 1, 2 at the output size
        ann, frame_index = sparse[small][None], [0]
        new_objects = None
        if cid == 'long':
            later = np.roll(ann[0], 6, axis=1)                      # the annotation of frame 6: both objects moved, id 6 enters
            later[OUT[0] // 2:OUT[0] // 2 + 40, 20:60] = 6
            ann, frame_index = np.stack([ann[0], later]), [0, 6]
            new_objects = {6: torch.from_numpy(np.where(later == 6, 3, 0).astype(np.uint8)).to(dev)}
        first = F.interpolate(torch.from_numpy(small)[None, None].float(), size=NET, mode='nearest')
        anns[cid] = ann
        clips.append((cid, f.to(dev), torch.from_numpy(ann).to(dev), frame_index))
        by_hand.append((cid, f.to(dev), first.to(dev), new_objects))
    got = {cid: (lab, proto) for cid, lab, proto in run_annotated_clips(_model(), iter(clips), rows=2, lookahead=2)}
    torch.cuda.synchronize()
    want = dict(run_clips(_model(), by_hand, rows=2, lookahead=2, out_hw=OUT))
    torch.cuda.synchronize()
    assert sorted(got) == ['long', 'short']
    assert got['short'][1].squeeze_idx == [0, 4, 9] and got['long'][1].squeeze_idx == [0, 4, 9, 6]
    assert got['long'][1].first_frame.tolist() == [0, 0, 6] and got['long'][1].new_frames == [6]
    for cid, n in (('short', 9), ('long', 14)):
        lab, proto = got[cid]
        assert tuple(lab.shape) == (n, *OUT) and torch.equal(lab, want[cid]), cid
        paths = [str(tmp_path / f'{cid}_{i:05d}.png') for i in range(n)]
        save_masks(lab, paths, proto.squeeze_idx)
        back = labels_from_pngs(paths, dev)
        # the engine may predict any of its max_obj_num ids: the table has all 256 entries, ids beyond the clip's objects -> 0
        original = torch.from_numpy(png.squeeze_lut(proto.squeeze_idx)).to(dev)
        assert torch.equal(back, original[lab.long()]), cid
    assert (got['long'][0][6:] == 3).any(), 'the new object never shows in the prediction'
    assert set(torch.unique(labels_from_pngs([str(tmp_path / 'long_00007.png')], dev)).tolist()) <= {0, 4, 9, 6}


def test_run_annotated_clips_refuses_too_many_objects(dev):
    from rmem_ocu_amd.evaluator import run_annotated_clips
    from test_hip_ragged_group import NET, OUT, _model
    ann = np.zeros((1, *OUT), dtype=np.uint8)
    for k in range(11):
        ann[0, 10 * k:10 * k + 5, 4:40] = 20 + k
    frames = torch.zeros(3, 3, *NET, device=dev)
    with pytest.raises(ValueError, match=r"'crowd'.*11 objects"):
        list(run_annotated_clips(_model(), [('crowd', frames, torch.from_numpy(ann).to(dev), None)], rows=2, lookahead=2))
    torch.cuda.synchronize()
