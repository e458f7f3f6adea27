"""The polygon fill on the MI355X against tests/polyfill_ref.py (the sequential restatement of the contract): whole stacks, exact
equality.  The round trip fills what the tracer emits and must return the stack it traced; the fractional cases aim at the seams
of the 32-bit plane words and at boxes that start and end inside a word; the stack sits between guard bytes and starts at any
byte, the output and the workspace are dirtied first.  References are computed once per case."""
import functools
import warnings

import numpy as np
import pytest
import torch

import census_ref
import polyfill_ref as P
import polygons_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
OFFSETS = (0, 1, 3, 13)
K = 10
CONTENTS = ['zero', 'full', 'blobs', 'speckle', 'noise', 'checker', 'hstripes', 'vstripes', 'serpentine', 'concentric', 'nest', 'others']
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 3, 5), (2, 67, 133), (3, 37, 131)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _content(shape, content):
    n, H, W = shape
    seed = n * 7919 + H * 131 + W
    if content == 'zero':
        a = np.zeros(shape, dtype=np.uint8)
    elif content == 'full':
        a = np.full(shape, 3, dtype=np.uint8)
    elif content == 'blobs':
        a = census_ref.blobs(seed, n, H, W)
    elif content == 'speckle':
        a = R.speckle(census_ref.blobs(seed, n, H, W), seed, 0.01, K)
    elif content == 'noise':
        a = R.noise(seed, n, H, W, 4)
    elif content == 'checker':
        a = R.checkerboard(n, H, W)
    elif content == 'hstripes':
        a = R.stripes(2 * n, H, W)[0::2]
    elif content == 'vstripes':
        a = R.stripes(2 * n, H, W)[1::2]
    elif content == 'serpentine':
        a = R.serpentine(n, H, W)
    elif content == 'concentric':
        a = R.concentric(n, H, W)
    elif content == 'nest':
        a = R.nest(n, H, W)
    else:                                                           # 'others': values above num_objs among the objects
        a = R.with_other_values(census_ref.blobs(seed, n, H, W), K, seed)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.shape == shape
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_round_trip_with_the_tracer(dev, shape, content):
    """fill(trace(labels)) == labels with the values above num_objs cleared, through both host products of the tracer"""
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd.evaluator import polygon_results
    a = _content(shape, content)
    want = np.where(a <= K, a, 0)
    d = torch.from_numpy(a.copy()).to(dev)
    for conn in (4, 8):
        got = polygons.fill_label_stack(polygons.trace_label_stack(d, K, conn), shape[1:], dev)
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape and np.array_equal(got.cpu().numpy(), want), (conn, 'trace_label_stack')
        got = polygons.fill_label_stack(polygon_results(d, K, holes='rings', connectivity=conn), shape[1:], dev)
        assert np.array_equal(got.cpu().numpy(), want), (conn, 'polygon_results')


# ---------------------------------------------------------------------------------------------------------------- the entry point, guarded
def _fill(dev, packed, offset=0, workspace_bytes=None):
    """rmem_polygon_fill_labels pass by pass into a stack between guard bytes that starts `offset` bytes past a 64-byte boundary;
    the stack and the workspace are 0xA5 first, the workspace is followed by guards too -> (labels, status) as numpy"""
    from rmem_ocu_amd import _lib, polygons
    n, H, W = packed.shape
    size, front = n * H * W, 64 + offset
    buf = torch.full((front + size + 64,), CANARY, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 64 == 0
    view = buf[front:front + size].view(n, H, W)
    plan = packed.passes(workspace_bytes)
    need = max(int(_lib.lib().rmem_polygon_fill_workspace_bytes(p.plane_words)) for p in plan)
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=dev)
    dc = packed.on_device(dev)
    dc.bits[:packed.buf.numel()].copy_(packed.buf)
    dc.status.fill_(-1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for p in plan:
        polygons.fill_pass(packed, dc, p, ws[:need], view, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:front] == CANARY).all() and (h[front + size:] == CANARY).all(), 'guard bytes around the stack'
    assert (ws[need:].cpu().numpy() == CANARY).all(), 'bytes beyond the workspace were written'
    return h[front:front + size].reshape(n, H, W).copy(), dc.status.cpu().numpy()


def _check(dev, frames, H, W, what, workspace_bytes=None):
    """frames[f] = [(value, [ring, ...])] through the guarded entry point at every byte offset, against the restatement"""
    from rmem_ocu_amd import polygons
    want = P.paint_stack(frames, H, W)
    packed = polygons.PackedPolygons(frames, (H, W))
    for offset in OFFSETS:
        got, status = _fill(dev, packed, offset, workspace_bytes)
        assert not status.any(), (what, offset, status)
        assert np.array_equal(got, want), (what, offset, np.argwhere(got != want)[:8])
    return packed, want


def _mid_word_box(H, W, value=5):
    """a box whose plane starts and ends inside a 32-bit word of the frame's columns"""
    return (value, [[(3.3, 0.2), (W - 2.5, 0.4), (W - 2.5, H - 0.2), (3.3, H - 0.3)]])


@functools.lru_cache(maxsize=None)
def _fractional(H, W):
    """five frames: 1 shape; none; 2 overlapping shapes; 255 shapes; a shape off the frame, an empty ring list, stars"""
    rng = np.random.default_rng(1000 * H + W)
    ring = lambda: P.random_polygon(rng, H, W)
    f0 = [(7, [ring(), ring()])]
    f2 = [_mid_word_box(H, W), (9, [ring()])]
    f3 = [(1 + k % 255, [ring()] if k % 5 else [ring(), P.star(rng, H, W)]) for k in range(254)] + [_mid_word_box(H, W, 77)]
    f4 = [(3, [[(-9.5, -9), (-2, -9), (-2, -1)]]), (4, []), (5, [P.star(rng, H, W), P.star(rng, H, W, 7)]), (6, [[(W + 1, 0), (W + 9, 0), (W + 5, H)]])]
    return [f0, [], f2, f3, f4]


@pytest.mark.parametrize('H', [1, 2, 19])
@pytest.mark.parametrize('W', [31, 32, 33, 63, 64, 65])
def test_fractional_polygons_at_the_word_seams(dev, W, H):
    frames = _fractional(H, W)
    assert [len(f) for f in frames] == [1, 0, 2, 255, 4]
    packed, want = _check(dev, frames, H, W, (H, W))
    assert packed.nshapes == 262
    flipped = [f[::-1] for f in frames]                              # the order decides where shapes overlap
    _check(dev, flipped, H, W, (H, W, 'reversed'))
    if H == 19:
        assert not np.array_equal(P.paint_stack(flipped, H, W), want)


def test_tie_cases(dev):
    cases = P.tie_cases()
    frames = [[(1 + k, rings)] for k, (_, rings) in enumerate(cases)]
    _check(dev, frames, 7, 9, 'ties, a frame each')
    _check(dev, [[(1 + k, rings) for k, (_, rings) in enumerate(cases)]], 7, 9, 'ties, one frame')


def test_triangle_fan_covers_every_pixel_exactly_once(dev):
    """the fan as a stack of k values: every pixel of the outline's fill holds exactly one triangle's value, whichever the order"""
    rng = np.random.default_rng(17)
    for j, (H, W) in enumerate(((19, 33), (7, 64), (18, 18), (1, 40), (19, 5), (13, 65))):
        outline, triangles = P.triangle_fan(rng, H, W, ('centre', 'corner', 'fraction')[j % 3])
        fan = [(1 + i, [t]) for i, t in enumerate(triangles)]
        packed, want = _check(dev, [fan, fan[::-1], [(200, [outline])]], H, W, ('fan', H, W))
        assert np.array_equal(want[0], want[1]) and np.array_equal(want[0] != 0, want[2] == 200)


def test_long_edges(dev):
    """one 480 x 854 frame: a 4-vertex box over the whole frame (two edges of 480 crossings each) under a thin sliver from corner to corner"""
    from rmem_ocu_amd import polygons
    H, W = 480, 854
    frames = [[(1, [[(0, 0), (W, 0), (W, H), (0, H)]]), (2, [[(0, 0), (1.5, 0), (W, H), (W - 1.5, H)]])]]
    want = P.paint_stack(frames, H, W)
    assert (want != 0).all() and 400 < int((want == 2).sum()) < 2000
    packed = polygons.PackedPolygons(frames, (H, W))
    assert packed.nedges == 4 and packed.crossings == 4 * H
    got, status = _fill(dev, packed, 13)
    assert not status.any() and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- memory discipline
def test_two_calls_and_passes_give_identical_bytes(dev):
    from rmem_ocu_amd import _lib, polygons
    H, W = 19, 65
    frames = _fractional(H, W)
    packed = polygons.PackedPolygons(frames, (H, W))
    first, second = _fill(dev, packed, 3), _fill(dev, packed, 3)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    one_frame = max(int(_lib.lib().rmem_polygon_fill_workspace_bytes(int(w))) for w in packed.frame_words)
    assert len(packed.passes(one_frame)) > 1 and len(packed.passes()) == 1
    by_pass = _fill(dev, packed, 3, one_frame)
    assert by_pass[0].tobytes() == first[0].tobytes() and by_pass[1].tobytes() == first[1].tobytes()
    out = torch.full((5, H, W), CANARY, dtype=torch.uint8, device=dev)
    polygons.fill_labels_into(packed, out, workspace_bytes=one_frame)
    assert np.array_equal(out.cpu().numpy(), first[0])
    with pytest.raises(_lib.RmemError, match=rf'at least the largest frame\'s need, {one_frame} bytes'):
        polygons.fill_labels_into(packed, out, workspace_bytes=one_frame - 1)


def test_two_packs_alternate_on_one_workspace(dev):
    """fill_labels_into shares one workspace per stream: a larger pack's planes never show in a smaller one's, and back"""
    from rmem_ocu_amd import polygons
    big, small = _fractional(19, 65), _fractional(2, 33)
    pb, ps = polygons.PackedPolygons(big, (19, 65)), polygons.PackedPolygons(small, (2, 33))
    wb, wsm = P.paint_stack(big, 19, 65), P.paint_stack(small, 2, 33)
    ob = torch.empty(5, 19, 65, dtype=torch.uint8, device=dev)
    os_ = torch.empty(5, 2, 33, dtype=torch.uint8, device=dev)
    for _ in range(2):
        ob.fill_(CANARY)
        polygons.fill_labels_into(pb, ob)
        os_.fill_(CANARY)
        polygons.fill_labels_into(ps, os_)
        pb.check(dev)
        ps.check(dev)
        assert np.array_equal(ob.cpu().numpy(), wb) and np.array_equal(os_.cpu().numpy(), wsm)
    empty = polygons.PackedPolygons([[], {}], (19, 65))               # a pack without any shape zero-fills
    oe = torch.full((2, 19, 65), CANARY, dtype=torch.uint8, device=dev)
    polygons.fill_labels_into(empty, oe)
    assert not oe.cpu().numpy().any()
    assert not polygons.fill_label_stack(empty, device=dev).cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------- status
def _status_clip():
    """two frames of two shapes each, every shape with crossings; shape k paints value k + 1"""
    H, W = 19, 45
    a, b = [(2.5, 1.2), (20.2, 2.0), (11.0, 17.5)], [(15, 3), (40.5, 3), (40.5, 16), (15, 16)]
    c, d = [(1, 1), (30, 2), (30, 18), (1, 15)], [(25.5, 0.5), (44, 9), (25.5, 18.5)]
    return [[(1, [a]), (2, [b])], [(3, [c]), (4, [d])]], H, W


def _corrupt(name, packed):
    """damage the pack after packing, before it reaches the device -> (status wanted per shape, the shapes that still paint)"""
    from rmem_ocu_amd import polygons
    table = packed.desc_bytes.numpy().view(polygons.SHAPE_DTYPE)
    ints = packed.buf.numpy().view(np.int32)
    E, S = packed.nedges, packed.nshapes
    DESC, PREFIX, EDGE = polygons.FILL_ST_DESC, polygons.FILL_ST_PREFIX, polygons.FILL_ST_EDGE
    if name == 'a decreasing frame':
        table[0]['frame'] = 1
        return [DESC, DESC, 0, 0]
    if name == 'a frame beyond the stack':
        table[3]['frame'] = 2
        return [0, 0, 0, DESC]
    if name == 'value 0':
        table[2]['value'] = 0
        return [0, 0, DESC, 0]
    if name == 'value 256':
        table[1]['value'] = 256
        return [0, DESC, 0, 0]
    if name == 'a box beyond the frame':
        table[3]['x1'] = packed.width + 1
        return [0, 0, 0, DESC]
    if name == 'a negative box':
        table[0]['y0'] = -1
        return [DESC, 0, 0, 0]
    if name == 'a plane beyond the workspace':
        table[1]['plane'] = packed.plane_words - 1
        return [0, DESC, 0, 0]
    if name == 'a plane before the pass':
        table[2]['plane'] = -4
        return [0, 0, DESC, 0]
    if name == 'an edge naming shape S':
        assert ints[5 * E - 1] == S - 1
        ints[5 * E - 1] = S
        return [0, 0, 0, DESC]
    if name == 'an edge naming shape -1':
        assert ints[4 * E] == 0
        ints[4 * E] = -1
        return [DESC, 0, 0, 0]
    if name == 'a crossing prefix that runs ahead':
        assert ints[4 * E] == 0 and ints[4 * E + 1] == 0              # edges 0 and 1 belong to shape 0
        ints[5 * E + 1] += 1
        return [PREFIX, 0, 0, 0]
    assert name == 'an edge coordinate beyond 2^28'
    assert ints[5 * E - 1] == S - 1
    ints[4 * (E - 1)] = 2 ** 28 + 1
    return [0, 0, 0, EDGE]


@pytest.mark.parametrize('name', ['a decreasing frame', 'a frame beyond the stack', 'value 0', 'value 256', 'a box beyond the frame', 'a negative box',
                                  'a plane beyond the workspace', 'a plane before the pass', 'an edge naming shape S', 'an edge naming shape -1',
                                  'a crossing prefix that runs ahead', 'an edge coordinate beyond 2^28'])
def test_a_corrupted_pack_sets_the_status_and_paints_nothing_for_the_shape(dev, name):
    """refusals, not faults: every index read from device memory is range-checked by the kernels before it is used"""
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    frames, H, W = _status_clip()
    packed = polygons.PackedPolygons(frames, (H, W))
    want_status = _corrupt(name, packed)
    want = P.paint_stack([[s for k, s in enumerate(fr) if not want_status[2 * f + k]] for f, fr in enumerate(frames)], H, W)
    got, status = _fill(dev, packed, 13)
    assert status.tolist() == want_status, (name, status)
    assert np.array_equal(got, want), name
    k = [i for i, s in enumerate(want_status) if s][0]
    with pytest.raises(RmemError, match=rf'polygon shape frame {k} .*\[shape {k}: frame {packed.where[k][0]}, value {packed.where[k][1]}\]'):
        packed.check(dev)


def test_fill_label_stack_raises_on_a_bad_status(dev):
    from rmem_ocu_amd import polygons
    from rmem_ocu_amd._lib import RmemError
    frames, H, W = _status_clip()
    packed = polygons.PackedPolygons(frames, (H, W))
    _corrupt('value 0', packed)
    with pytest.raises(RmemError, match=r'status 1: bad shape table entry.*\[shape 2: frame 1, value 3\]'):
        polygons.fill_label_stack(packed, device=dev)


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_fill_labels_into_makes_no_host_sync(dev, monkeypatch):
    """nothing in polygons.fill_labels_into waits for the device: every synchronising call raises meanwhile; fill_label_stack,
    which reads the status words back, is the control that the patches bite"""
    from rmem_ocu_amd import _lib, polygons
    H, W = 19, 65
    frames = _fractional(H, W)
    want = P.paint_stack(frames, H, W)
    packed = polygons.PackedPolygons(frames, (H, W))
    out = torch.full((5, H, W), CANARY, dtype=torch.uint8, device=dev)
    polygons.fill_labels_into(packed, out)                           # the pack's device copy and the workspace exist now
    torch.cuda.synchronize()
    one_frame = max(int(_lib.lib().rmem_polygon_fill_workspace_bytes(int(w))) for w in packed.frame_words)
    assert len(packed.passes(one_frame)) > 1
    out.fill_(CANARY)

    def refuse(*a, **k):
        raise AssertionError('a host synchronisation inside polygons')

    with monkeypatch.context() as m:
        for owner, name in ((torch.Tensor, 'item'), (torch.Tensor, 'cpu'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'),
                            (torch.Tensor, '__bool__'), (torch.Tensor, '__int__'), (torch.cuda, 'synchronize'),
                            (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
            m.setattr(owner, name, refuse)
        with pytest.raises(AssertionError, match='host synchronisation'):
            polygons.fill_label_stack(packed, device=dev)
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                         # "a prototype feature": it may miss a sync, the patches above do not
            torch.cuda.set_sync_debug_mode('error')
        try:
            polygons.fill_labels_into(packed, out)
            polygons.fill_labels_into(packed, out, workspace_bytes=one_frame)
        finally:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    packed.check(dev)
    assert np.array_equal(out.cpu().numpy(), want)


def test_labels_from_polygons_feeds_the_clip_protocol(dev):
    """two tracks, one of them missing on some frames: the stack, the ids, and protocol.clip_protocol downstream"""
    from rmem_ocu_amd.evaluator import labels_from_polygons
    from rmem_ocu_amd.protocol import clip_protocol
    H, W = 24, 40

    def box(x, y, w, h):
        return [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]

    frames = [{'dog': box(2.5, 3, 10, 8)}, {'dog': box(3.5, 3, 10, 8), 'cat': {'exterior': box(20, 10, 12.5, 9), 'holes': [box(24, 13, 3, 3)]}},
              {'cat': [box(21, 10, 12, 9)]}, {'dog': box(5.5, 4, 10, 8), 'cat': box(22, 10, 12, 9)}]
    labels, ids = labels_from_polygons(frames, (H, W), dev)
    assert ids == ['cat', 'dog'] and labels.dtype == torch.uint8 and tuple(labels.shape) == (4, H, W) and labels.device == dev
    value = {'cat': 1, 'dog': 2}
    listed = []
    for fr in frames:
        shapes = []
        for k, s in fr.items():
            rings = [s['exterior']] + s['holes'] if isinstance(s, dict) else (s if isinstance(s[0], list) else [s])
            shapes.append((value[k], rings))
        listed.append(shapes)
    want = P.paint_stack(listed, H, W)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want) and set(np.unique(got[0])) == {0, 2} and set(np.unique(got[2])) == {0, 1}
    assert got[1, 14, 25] == 0 and got[1, 11, 25] == 1                # the hole
    proto, first, new = clip_protocol(labels)
    assert proto.num_objs == 2 and proto.squeeze_idx == [0, 2, 1] and proto.first_frame.tolist() == [0, 1] and proto.new_frames == [1]
    assert np.array_equal(first.cpu().numpy(), np.where(want[0] == 2, 1, 0)) and list(new) == [1]
    assert np.array_equal(new[1].cpu().numpy(), np.where(want[1] == 1, 2, 0))
    only, ids = labels_from_polygons(frames, (H, W), dev, ids=['dog'])
    assert ids == ['dog'] and np.array_equal(only.cpu().numpy(), np.where(want == 2, 1, 0))
