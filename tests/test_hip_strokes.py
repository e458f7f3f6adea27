"""The stroke rasteriser on the MI355X against tests/strokes_ref.py (the sequential restatement of the contract): whole stacks,
exact equality.  The small shapes aim at the 16-byte pieces of the painter and at rows of one, two and many pixels; the stack sits
between guard bytes and starts at any byte, the output and the workspace are dirtied first.  References are computed once per case."""
import functools
import warnings

import numpy as np
import pytest
import torch

import strokes_ref as S

pytestmark = pytest.mark.gpu

CANARY = 0xA5
OFFSETS = (0, 1, 3, 13)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------------------- the entry point, guarded
def _draw(dev, packed, offset=0, workspace_bytes=None, base=None):
    """rmem_stroke_draw_labels pass by pass into a stack between guard bytes that starts `offset` bytes past a 64-byte boundary;
    the stack (or base, drawn over) and the workspace are 0xA5 first, the workspace is followed by guards too -> (labels, status)"""
    from rmem_ocu_amd import _lib, strokes
    n, H, W = packed.shape
    size, front = n * H * W, 64 + offset
    buf = torch.full((front + size + 64,), CANARY, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 64 == 0
    view = buf[front:front + size].view(n, H, W)
    if base is not None:
        view.copy_(torch.from_numpy(base))
    plan = packed.passes(workspace_bytes)
    need = max(int(_lib.lib().rmem_stroke_workspace_bytes(p.slots, H, W)) for p in plan)
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=dev)
    dc = packed.on_device(dev)
    dc.bits[:packed.buf.numel()].copy_(packed.buf)
    dc.status.fill_(-1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for p in plan:
        strokes.draw_pass(packed, dc, p, ws[:need], view, base is not None, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:front] == CANARY).all() and (h[front + size:] == CANARY).all(), 'guard bytes around the stack'
    assert (ws[need:].cpu().numpy() == CANARY).all(), 'bytes beyond the workspace were written'
    return h[front:front + size].reshape(n, H, W).copy(), dc.status.cpu().numpy()


def _check(dev, frames, H, W, want, what, offsets=OFFSETS, workspace_bytes=None, base=None):
    from rmem_ocu_amd import strokes
    packed = strokes.PackedStrokes(frames, (H, W))
    for offset in offsets:
        got, status = _draw(dev, packed, offset, workspace_bytes, base)
        assert not status.any(), (what, offset, status)
        assert np.array_equal(got, want), (what, offset, np.argwhere(got != want)[:8])
    return packed


@functools.lru_cache(maxsize=None)
def _small(H, W):
    """(frames, their pixel sets): six frames of 1, 0, 2 overlapping, 4, 255 and 3 strokes, every radius of the issue among them"""
    seed = 1000 * H + W
    cross = [{'value': 5, 'path': [(1.2, 0.3), (W - 2.5, H - 0.6)], 'radius': 2.5}, {'value': 9, 'path': [(W - 1.0, 0.0), (0.4, H - 1.0)], 'radius': 1}]
    frames = [S.random_strokes(seed, H, W, 1, radii=(7,)), [], cross, S.random_strokes(seed + 1, H, W, 4),
              S.random_strokes(seed + 2, H, W, 255, k=2, step=3.0), S.random_strokes(seed + 3, H, W, 3, radii=(0.4, 0, 0))]
    return frames, S.stroke_sets(frames, H, W)


@pytest.mark.parametrize('H', [1, 2, 19])
@pytest.mark.parametrize('W', [31, 32, 33, 63, 64, 65])
def test_seeded_strokes_at_the_piece_seams(dev, W, H):
    frames, sets = _small(H, W)
    assert [len(f) for f in frames] == [1, 0, 2, 4, 255, 3]
    assert {s['radius'] for f in frames for s in f} == {0, 0.4, 1, 2.5, 7}
    want = S.paint_sets(sets, H, W)
    packed = _check(dev, frames, H, W, want, (H, W))
    assert packed.nstrokes == 265 and packed.stroked.tolist() == [0, 2, 3, 4, 5]
    flipped, flipped_sets = [f[::-1] for f in frames], [s[::-1] for s in sets]      # the order decides where strokes overlap
    want_flipped = S.paint_sets(flipped_sets, H, W)
    _check(dev, flipped, H, W, want_flipped, (H, W, 'reversed'), offsets=(3,))
    if H == 19:
        assert not np.array_equal(want_flipped[2], want[2]) and want[2].any()


def test_a_stack_whose_middle_frame_has_no_strokes(dev):
    H, W = 19, 33
    frames = [S.random_strokes(41, H, W, 3), [], S.random_strokes(42, H, W, 2)]
    want = S.paint_stack(frames, H, W)
    assert want[0].any() and not want[1].any() and want[2].any()
    packed = _check(dev, frames, H, W, want, 'middle frame empty')
    assert packed.stroked.tolist() == [0, 2] and packed.passes()[0].slots == 2


def test_over_keeps_every_uncovered_byte(dev):
    H, W = 19, 65
    frames, sets = _small(H, W)
    base = np.random.default_rng(3).integers(0, 256, size=(6, H, W), dtype=np.uint8)
    want = S.paint_sets(sets, H, W, base)
    covered = S.paint_sets([[(1, px) for _, px in fr] for fr in sets], H, W) != 0
    assert np.array_equal(want[~covered], base[~covered]) and np.array_equal(want[1], base[1]) and (want != base).sum() > 100
    _check(dev, frames, H, W, want, 'over', base=base)
    one_map = H * W * 4 + 15 & ~15
    _check(dev, frames, H, W, want, 'over, a frame per pass', offsets=(13,), workspace_bytes=one_map, base=base)


def test_tie_cases(dev):
    for name, stroke, H, W, pixels in S.tie_cases():
        want = S.mask_of(pixels, H, W).astype(np.uint8)[None]
        _check(dev, [[stroke]], H, W, want, name, offsets=(0, 13))


def test_a_corner_to_corner_stroke_in_a_large_frame(dev):
    """one 480 x 854 frame: a diagonal from corner to corner as a hairline (one sample per column) and at r = 256 (every row of
    the frame one work item, its columns narrowed), each under a dot"""
    from rmem_ocu_amd import strokes
    H, W = 480, 854
    diag = [(0, 0), (W - 1, H - 1)]
    dot = {'value': 9, 'path': [(400, 200)], 'radius': 3}
    frames = [[{'value': 1, 'path': diag, 'radius': 0}, dot], [{'value': 2, 'path': diag, 'radius': 256}, dot]]
    want = np.zeros((2, H, W), dtype=np.uint8)
    for y, x in S.hairline_pixels(S.points(diag), H, W):
        want[0, y, x] = 1
    want[1][S.brush_mask_large(S.points(diag), 256 * 256, H, W)] = 2
    for f in (0, 1):
        want[f][S.brush_mask_large(S.points(dot['path']), 3 * 256, H, W)] = 9
    assert int((want[0] == 1).sum()) == W and 0.8 * H * W < int((want[1] == 2).sum()) < H * W and int((want == 9).sum()) == 2 * 29
    packed = strokes.PackedStrokes(frames, (H, W))
    assert packed.nsegs == 4 and packed.seg_first.tolist() == [0, W + 2, W + 2 + 7, W + 9 + H, W + 9 + H + 7]
    got, status = _draw(dev, packed, 13)
    assert not status.any() and np.array_equal(got, want), np.argwhere(got != want)[:8]


# ---------------------------------------------------------------------------------------------------------------- memory discipline
def test_two_calls_and_passes_give_identical_bytes(dev):
    from rmem_ocu_amd import _lib, strokes
    H, W = 19, 65
    frames, sets = _small(H, W)
    packed = strokes.PackedStrokes(frames, (H, W))
    first, second = _draw(dev, packed, 3), _draw(dev, packed, 3)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    one_map = int(_lib.lib().rmem_stroke_workspace_bytes(1, H, W))
    assert len(packed.passes(one_map)) == 5 and len(packed.passes()) == 1
    by_pass = _draw(dev, packed, 3, one_map)
    assert by_pass[0].tobytes() == first[0].tobytes() and by_pass[1].tobytes() == first[1].tobytes()
    out = torch.full((6, H, W), CANARY, dtype=torch.uint8, device=dev)
    strokes.draw_labels_into(packed, out, workspace_bytes=one_map)
    assert np.array_equal(out.cpu().numpy(), first[0])
    with pytest.raises(_lib.RmemError, match=rf'at least one frame\'s need, {one_map} bytes'):
        strokes.draw_labels_into(packed, out, workspace_bytes=one_map - 1)


def test_two_packs_alternate_on_one_workspace(dev):
    """draw_labels_into shares one workspace per stream: a larger pack's owner maps never show in a smaller one's, and back"""
    from rmem_ocu_amd import strokes
    (big, bs), (small, ss) = _small(19, 65), _small(2, 33)
    pb, ps = strokes.PackedStrokes(big, (19, 65)), strokes.PackedStrokes(small, (2, 33))
    wb, wsm = S.paint_sets(bs, 19, 65), S.paint_sets(ss, 2, 33)
    ob = torch.empty(6, 19, 65, dtype=torch.uint8, device=dev)
    os_ = torch.empty(6, 2, 33, dtype=torch.uint8, device=dev)
    for _ in range(2):
        ob.fill_(CANARY)
        strokes.draw_labels_into(pb, ob)
        os_.fill_(CANARY)
        strokes.draw_labels_into(ps, os_)
        pb.check(dev)
        ps.check(dev)
        assert np.array_equal(ob.cpu().numpy(), wb) and np.array_equal(os_.cpu().numpy(), wsm)
    empty = strokes.PackedStrokes([[], []], (19, 65))                  # a pack without any stroke zero-fills a fresh stack
    oe = torch.full((2, 19, 65), CANARY, dtype=torch.uint8, device=dev)
    strokes.draw_labels_into(empty, oe, over=True)
    assert (oe.cpu().numpy() == CANARY).all()
    strokes.draw_labels_into(empty, oe)
    assert not oe.cpu().numpy().any()
    assert not strokes.draw_label_stack(empty, device=dev).cpu().numpy().any()
    base = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(6, 19, 65), dtype=np.uint8)).to(dev)
    kept = base.clone()
    got = strokes.draw_label_stack(big, (19, 65), dev, base=base)
    assert np.array_equal(got.cpu().numpy(), S.paint_sets(bs, 19, 65, base.cpu().numpy())) and torch.equal(base, kept)


# ---------------------------------------------------------------------------------------------------------------- status
def _status_clip():
    """two frames of two strokes each, every stroke of two segments inside the frame; stroke k draws value k + 1"""
    H, W = 19, 45
    return [[(1, [(2.5, 1.2), (20.2, 2.0), (11.0, 17.5)], 1.5), (2, [(15, 3), (40.5, 3), (40.5, 16)], 0)],
            [(3, [(1, 1), (30, 2), (30, 16)], 2.5), (4, [(25.5, 0.5), (44, 9), (25.5, 18.5)], 0)]], H, W


DAMAGE = ['a decreasing frame', 'a frame beyond the stack', 'value 256', 'value -1', 'radius 65537', 'radius -1', 'a box beyond the frame',
          'a negative box', 'a slot beyond the pass', 'the slot of another frame', 'a segment naming stroke S', 'a segment naming stroke -1',
          'a prefix that runs ahead', 'a prefix that does not start at the pass\'s first item', 'a coordinate beyond 2^28',
          'a hairline against its major axis', 'a stroke box smaller than its segments']


def _corrupt(name, packed):
    """damage the pack after packing, before it reaches the device -> the status wanted per stroke"""
    from rmem_ocu_amd import strokes
    table = packed.desc_bytes.numpy().view(strokes.STROKE_DTYPE)
    ints = packed.buf.numpy().view(np.int32)
    E, N = packed.nsegs, packed.nstrokes
    DESC, PREFIX, SEGMENT = strokes.ST_DESC, strokes.ST_PREFIX, strokes.ST_SEGMENT
    assert E == 8 and N == 4 and ints[4 * E:5 * E].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    if name == 'a decreasing frame':
        table[0]['frame'] = 1
        return [DESC, DESC, 0, 0]
    if name == 'a frame beyond the stack':
        table[3]['frame'] = 2
        return [0, 0, 0, DESC]
    if name in ('value 256', 'value -1'):
        table[1]['value'] = int(name.split()[1])
        return [0, DESC, 0, 0]
    if name in ('radius 65537', 'radius -1'):
        table[2]['radius'] = int(name.split()[1])
        return [0, 0, DESC, 0]
    if name == 'a box beyond the frame':
        table[3]['x1'] = packed.width + 1
        return [0, 0, 0, DESC]
    if name == 'a negative box':
        table[0]['y0'] = -1
        return [DESC, 0, 0, 0]
    if name == 'a slot beyond the pass':
        table[3]['slot'] = 2
        return [0, 0, 0, DESC]
    if name == 'the slot of another frame':
        table[0]['slot'] = 1
        return [DESC, 0, 0, 0]
    if name == 'a segment naming stroke S':
        ints[5 * E - 1] = N
        return [0, 0, 0, DESC]                                          # on the pass's last stroke, the nearest to the name
    if name == 'a segment naming stroke -1':
        ints[4 * E] = -1
        return [DESC, 0, 0, 0]
    if name == 'a prefix that runs ahead':
        ints[5 * E + 1] += 1                                            # between the two segments of stroke 0
        return [PREFIX, 0, 0, 0]
    if name == 'a prefix that does not start at the pass\'s first item':
        ints[5 * E] = 1
        return [PREFIX, 0, 0, 0]
    if name == 'a coordinate beyond 2^28':
        ints[4 * (E - 1)] = 2 ** 28 + 1
        return [0, 0, 0, SEGMENT]
    if name == 'a hairline against its major axis':
        seg = ints[4 * (E - 1):4 * E].copy()
        ints[4 * (E - 1):4 * E] = seg[[2, 3, 0, 1]]
        return [0, 0, 0, SEGMENT]
    assert name == 'a stroke box smaller than its segments'
    table[2]['x1'] -= 1
    return [0, 0, SEGMENT, 0]


@pytest.mark.parametrize('name', DAMAGE)
def test_a_corrupted_pack_sets_the_status_and_draws_nothing_for_the_stroke(dev, name):
    """refusals, not faults: every index read from device memory is range-checked by the kernels before it is used"""
    from rmem_ocu_amd import strokes
    from rmem_ocu_amd._lib import RmemError
    frames, H, W = _status_clip()
    packed = strokes.PackedStrokes(frames, (H, W))
    want_status = _corrupt(name, packed)
    want = S.paint_stack([[s for k, s in enumerate(fr) if not want_status[2 * f + k]] for f, fr in enumerate(frames)], H, W)
    got, status = _draw(dev, packed, 13)
    assert status.tolist() == want_status, (name, status)
    assert np.array_equal(got, want), name
    k = [i for i, s in enumerate(want_status) if s][0]
    with pytest.raises(RmemError, match=rf'stroke frame {k} .*\[stroke {k}: frame {packed.where[k][0]}, value {packed.where[k][1]}\]'):
        packed.check(dev)


def test_draw_label_stack_raises_on_a_bad_status(dev):
    from rmem_ocu_amd import strokes
    from rmem_ocu_amd._lib import RmemError
    frames, H, W = _status_clip()
    packed = strokes.PackedStrokes(frames, (H, W))
    _corrupt('value 256', packed)
    with pytest.raises(RmemError, match=r'status 1: bad stroke table entry.*\[stroke 1: frame 0, value 2\]'):
        strokes.draw_label_stack(packed, device=dev)


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_draw_labels_into_makes_no_host_sync(dev, monkeypatch):
    """nothing in strokes.draw_labels_into waits for the device: every synchronising call raises meanwhile; draw_label_stack,
    which reads the status words back, is the control that the patches bite"""
    from rmem_ocu_amd import _lib, strokes
    H, W = 19, 65
    frames, sets = _small(H, W)
    want = S.paint_sets(sets, H, W)
    packed = strokes.PackedStrokes(frames, (H, W))
    out = torch.full((6, H, W), CANARY, dtype=torch.uint8, device=dev)
    strokes.draw_labels_into(packed, out)                            # the pack's device copy and the workspace exist now
    torch.cuda.synchronize()
    one_map = int(_lib.lib().rmem_stroke_workspace_bytes(1, H, W))
    out.fill_(CANARY)

    def refuse(*a, **k):
        raise AssertionError('a host synchronisation inside strokes')

    with monkeypatch.context() as m:
        for owner, name in ((torch.Tensor, 'item'), (torch.Tensor, 'cpu'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'),
                            (torch.Tensor, '__bool__'), (torch.Tensor, '__int__'), (torch.cuda, 'synchronize'),
                            (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
            m.setattr(owner, name, refuse)
        with pytest.raises(AssertionError, match='host synchronisation'):
            strokes.draw_label_stack(packed, device=dev)
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                         # "a prototype feature": it may miss a sync, the patches above do not
            torch.cuda.set_sync_debug_mode('error')
        try:
            strokes.draw_labels_into(packed, out)
            strokes.draw_labels_into(packed, out, workspace_bytes=one_map)
            strokes.draw_labels_into(packed, out, over=True)
        finally:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    packed.check(dev)
    assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _pair():
    """a 2 x 37 x 131 prediction and annotation that disagree in blobs deep enough for scribbles"""
    n, H, W = 2, 37, 131
    gt = np.zeros((n, H, W), dtype=np.uint8)
    gt[:, 5:30, 10:50], gt[:, 8:33, 70:120] = 1, 2
    pred = gt.copy()
    pred[0, 5:30, 10:28], pred[1, 8:20, 70:120] = 0, 0                # false negatives of objects 1 and 2
    pred[0, 8:33, 55:70], pred[1, 0:5, 0:40] = 2, 1                   # false positives
    return pred, gt


def test_scribbles_draw_back_onto_their_paths(dev):
    from rmem_ocu_amd import evaluator
    pred, gt = (torch.from_numpy(a).to(dev) for a in _pair())
    n, H, W = pred.shape
    scribbles = evaluator.next_scribbles(pred, gt, 2)
    assert sum(len(f) for f in scribbles) >= 3 and any(not s['positive'] for f in scribbles for s in f.values())
    seeds = evaluator.seeds_from_scribbles(scribbles, (H, W), dev, radius=0, background=7)
    assert seeds.dtype == torch.uint8 and tuple(seeds.shape) == (n, H, W) and seeds.device == dev
    on_paths = np.zeros((n, H, W), dtype=bool)
    for f, fr in enumerate(scribbles):
        for s in fr.values():
            on_paths[f, s['path'][:, 0], s['path'][:, 1]] = True
    assert np.array_equal(seeds.cpu().numpy() != 0, on_paths) and on_paths.sum() > 20


def test_clicks_draw_onto_themselves_and_one_round_runs(dev):
    from rmem_ocu_amd import evaluator
    pred, gt = (torch.from_numpy(a).to(dev) for a in _pair())
    n, H, W = pred.shape
    clicks = evaluator.next_clicks(pred, gt, 2)
    seeds = evaluator.seeds_from_clicks(clicks, (H, W), dev, radius=0, background=7)
    on_clicks = np.zeros((n, H, W), dtype=bool)
    for f in range(n):
        for y, x, positive, d2 in clicks[f]:
            if y >= 0:
                on_clicks[f, y, x] = True
    assert np.array_equal(seeds.cpu().numpy() != 0, on_clicks) and 2 <= on_clicks.sum() <= 4
    seeds = evaluator.seeds_from_scribbles(evaluator.next_scribbles(pred, gt, 2), (H, W), dev, radius=1.5, background=7)
    labels = evaluator.labels_from_seeds(seeds, background=7)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n, H, W) and set(np.unique(labels.cpu().numpy())) <= {0, 1, 2}
    doc = {'scribbles': [[{'path': [[0.1, 0.2], [0.5, 0.5], [0.9, 0.4]], 'object_id': 1}], []]}
    got = evaluator.labels_from_scribbles(doc, (H, W), dev, radius=2)
    path = np.trunc(np.array(doc['scribbles'][0][0]['path']) * (W - 1, H - 1))
    assert np.array_equal(got.cpu().numpy(), S.paint_stack([[(1, path, 2)], []], H, W))
