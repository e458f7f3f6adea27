"""The pair boundary census on the MI355X against tests/pair_boundary_ref.py: exact integer equality everywhere.  The workspace is
dirtied first, all three outputs are dirtied first and followed by guard ints, both stacks sit between guard bytes and start at
any byte.  Then the yardsticks that need no slow reference (the diagonal scorer), the passes, streams, and what the evaluator
builds on the tables: score_clip_objects and score_unsupervised_clip."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import boundary_ref
import census_ref
import pair_boundary_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
TINY = [(1, 1, 1), (1, 1, 17), (2, 3, 5)]
SMALL = TINY + [(3, 17, 33), (2, 37, 131)]           # a partial word and fewer rows than a tile; three words and three row tiles
WIDE = (1, 40, 1100)                                  # 18 words: two x-tiles, the halo word crosses the tile edge
TALL = (1, 150, 200)                                  # room for a radius of 63
CONTENTS = ['zero', 'identical', 'shifted', 'different', 'noise', 'void', 'above', 'pixels', 'edges']
OFFSETS = [(0, 0), (1, 1), (3, 13), (13, 0), (0, 7)]
NUMS = [(1, 1), (5, 3), (31, 31), (32, 32), (64, 64), (65, 70)]


def _sid(s):
    return 'x'.join(map(str, s))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _content(shape, content, num_a, num_b):
    """(a, b) of one (shape, content) for (num_a, num_b) objects: computed once, shared, read only"""
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W + 17 * num_a + num_b)
    blobs_a = census_ref.blobs(H * W + n, n, H, W, ids=tuple(range(1, num_a + 1)))
    if content == 'zero':
        a, b = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    elif content == 'identical':
        a, b = blobs_a, np.where(blobs_a <= num_b, blobs_a, 0).astype(np.uint8)
    elif content == 'shifted':                                     # blobs against themselves moved by (2, 3)
        a, b = blobs_a, np.roll(blobs_a, (2, 3), axis=(1, 2))
    elif content == 'different':
        a, b = blobs_a, census_ref.blobs(H * W + n + 1, n, H, W, ids=tuple(range(1, num_b + 1)))
    elif content == 'noise':                                       # num + 1 ids each: every word holds every id
        a = rng.integers(0, min(num_a + 1, 255) + 1, shape).astype(np.uint8)
        b = rng.integers(0, min(num_b + 1, 255) + 1, shape).astype(np.uint8)
    elif content == 'void':                                        # 10 % of b is 255
        a, b = blobs_a, np.roll(blobs_a, (1, 2), axis=(1, 2))
        b[rng.random(shape) < 0.1] = 255
    elif content == 'above':                                       # both stacks hold values past num, 255 (void) among b's
        a, b = blobs_a.copy(), np.roll(blobs_a, (2, 3), axis=(1, 2))
        hit = rng.random(shape) < 0.2
        a[hit] = rng.integers(min(num_a + 1, 255), 256, shape).astype(np.uint8)[hit]
        hit = rng.random(shape) < 0.2
        b[hit] = rng.integers(min(num_b + 1, 255), 256, shape).astype(np.uint8)[hit]
    elif content == 'pixels':                                      # one-pixel objects
        a, b = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
        for t, num in ((a, num_a), (b, num_b)):
            for v in range(1, num + 1):
                t[rng.integers(n), rng.integers(H), rng.integers(W)] = v
    else:                                                          # 'edges': the last row, the last column, the corner pixel
        a, b = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
        a[:, -1, :] = 1
        a[:, :, -1] = min(2, num_a)
        a[:, -1, -1] = min(3, num_a)
        b[:, -1, W // 2:] = 1
        b[:, H // 2:, -1] = min(2, num_b)
        b[:, -1, -1] = min(3, num_b) if n > 1 else 0
        b[0, 0, 0] = 1
    for t in (a, b):
        t.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(shape, content, num_a, num_b, void, bound_th):
    a, b = _content(shape, content, num_a, num_b)
    want = ref.tables(a, b, num_a, num_b, void, bound_th)
    for t in want:
        t.setflags(write=False)
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


def _counts(dev, a, b, num_a, num_b, void, bound_th, offsets=(0, 0), frames_per_pass=None):
    """rmem_pair_boundary_counts on guarded copies of a and b, a workspace full of 0xA5, outputs full of 0xA5 followed by guard ints"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = a.shape
    abuf, aview, afront = _guarded(dev, a, offsets[0])
    bbuf, bview, bfront = _guarded(dev, b, offsets[1])
    radius = L.rmem_boundary_radius(H, W, float(bound_th))
    assert radius == boundary_ref.radius(H, W, bound_th)
    per_frame = L.rmem_pair_boundary_workspace_bytes(1, H, W, num_a, num_b)
    assert per_frame == (num_a + num_b + 2) * H * ((W + 63) // 64) * 8
    nbytes = per_frame * (n if frames_per_pass is None else frames_per_pass)
    ws = torch.full((nbytes + 64,), CANARY, dtype=torch.uint8, device=dev)
    sizes = (n * (num_a + 1) * (num_b + 1) * 2, n * (num_a + 1), n * (num_b + 1))
    outs = [torch.full((s + 64,), CANARY32, dtype=torch.int32, device=dev) for s in sizes]
    _lib.check(L.rmem_pair_boundary_counts(aview.data_ptr(), bview.data_ptr(), n, H, W, num_a, num_b, -1 if void is None else void,
                                           radius, ws.data_ptr(), nbytes, outs[1].data_ptr(), outs[2].data_ptr(), outs[0].data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), 'rmem_pair_boundary_counts')
    torch.cuda.synchronize()
    assert _guards_intact(abuf, afront, a.size) and _guards_intact(bbuf, bfront, b.size), 'guard bytes around the stacks'
    assert np.array_equal(abuf[afront:afront + a.size].cpu().numpy(), a.reshape(-1)), 'a is read only'
    assert np.array_equal(bbuf[bfront:bfront + b.size].cpu().numpy(), b.reshape(-1)), 'b is read only'
    assert (ws[nbytes:].cpu().numpy() == CANARY).all(), 'bytes beyond the workspace were written'
    host = [o.cpu().numpy() for o in outs]
    for o, s in zip(host, sizes):
        assert (o[s:] == CANARY32).all(), 'ints beyond an output were written'
    return (host[0][:sizes[0]].reshape(n, num_a + 1, num_b + 1, 2), host[1][:sizes[1]].reshape(n, num_a + 1),
            host[2][:sizes[2]].reshape(n, num_b + 1))


def _check(dev, shape, content, num_a, num_b, void=255, bound_th=2, offsets=(0, 0), frames_per_pass=None):
    a, b = _content(shape, content, num_a, num_b)
    got = _counts(dev, a, b, num_a, num_b, void, bound_th, offsets, frames_per_pass)
    want = _ref(shape, content, num_a, num_b, void, bound_th)
    for g, w, name in zip(got, want, ('match', 'bnd_a', 'bnd_b')):
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, content, num_a, num_b, offsets, np.argwhere(g != w)[:8])
    assert not got[0][:, 0].any() and not got[0][:, :, 0].any() and not got[1][:, 0].any() and not got[2][:, 0].any()
    return got


# noise is for the three smallest shapes: every word holds every id there already
@pytest.mark.parametrize('shape,content', [(s, c) for s in SMALL for c in CONTENTS if c != 'noise' or s in TINY],
                         ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_contents(dev, shape, content):
    _check(dev, shape, content, 5, 3)
    _check(dev, shape, content, 5, 3, void=None, bound_th=1)


@pytest.mark.parametrize('bound_th', [1, 2, 8, 63, 0.008])
def test_radii(dev, bound_th):
    """every radius on three words x three row tiles and on two x-tiles; 63 also where it fits inside the frame"""
    for shape in ((2, 37, 131), WIDE) + ((TALL,) if bound_th == 63 else ()):
        for content in ('shifted', 'different', 'void'):
            _check(dev, shape, content, 5, 3, bound_th=bound_th)


def test_wide_and_tall_contents(dev):
    for shape in (WIDE, TALL):
        for content in ('identical', 'above', 'pixels', 'edges'):
            _check(dev, shape, content, 5, 3, bound_th=8)


@pytest.mark.parametrize('nums', NUMS, ids=lambda p: f'{p[0]}x{p[1]}')
def test_numbers_of_objects(dev, nums):
    """up to the old scorer's 31, the first case beyond it, and across the lane count"""
    for shape in ((3, 17, 33), (2, 37, 131)):
        for content in ('shifted', 'different', 'void', 'above'):
            _check(dev, shape, content, nums[0], nums[1], offsets=(3, 13))


@functools.lru_cache(maxsize=None)
def _grid255():
    """48 x 320: a 16 x 16 grid of cells of 3 x 20 pixels holding ids 0..255, against itself rolled by (1, 7)"""
    a = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16), 3, axis=0), 20, axis=1)[None]
    b = np.roll(a, (1, 7), axis=(1, 2))
    want = ref.tables(a, b, 255, 255, None, 3)
    return a, b, want


def test_255_objects_on_both_sides(dev):
    a, b, want = _grid255()
    assert (want[1][0, 1:] > 0).all() and (want[2][0, 1:] > 0).all()
    off = want[0][0, 1:, 1:].any(axis=2) & ~np.eye(255, dtype=bool)
    assert off.sum() > 1000, 'many pairs off the diagonal match'
    got = _counts(dev, a, b, 255, 255, None, 3, (1, 1))
    for g, w in zip(got, want):
        assert np.array_equal(g, w), np.argwhere(g != w)[:8]


@pytest.mark.parametrize('offsets', OFFSETS, ids=lambda o: f'{o[0]}+{o[1]}')
def test_byte_offsets(dev, offsets):
    for shape in SMALL:
        _check(dev, shape, 'void', 5, 3, offsets=offsets)
        _check(dev, shape, 'edges', 5, 3, offsets=offsets)


@pytest.mark.parametrize('shape', [(3, 17, 33), (2, 37, 131)], ids=_sid)
def test_one_frame_per_pass(dev, shape):
    """a workspace of exactly one frame's planes against one for the whole stack: identical outputs"""
    for content, nums in (('void', (5, 3)), ('different', (65, 70))):
        whole = _check(dev, shape, content, *nums)
        single = _check(dev, shape, content, *nums, frames_per_pass=1)
        assert all(np.array_equal(x, y) for x, y in zip(whole, single))
    if shape[0] == 3:
        _check(dev, shape, 'void', 5, 3, frames_per_pass=2)         # a last pass of fewer frames


# ------------------------------------------------------------------------------------------------------------------ yardsticks
def _device(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]


def _equals_the_diagonal_scorer(dev, a, b, num):
    from rmem_ocu_amd.evaluator import clip_counts
    from rmem_ocu_amd.pairs import pair_boundary_counts
    ad, bd = _device(dev, a, b)
    match, bnd_a, bnd_b = (t.cpu().numpy() for t in pair_boundary_counts(ad, bd, num, num))
    counts = clip_counts(ad, bd, num + 1, 255).cpu().numpy()
    d = np.arange(num + 1)
    assert np.array_equal(bnd_a, counts[:, :, 0]) and np.array_equal(bnd_b, counts[:, :, 1])
    assert np.array_equal(match[:, d, d, 0], counts[:, :, 2]) and np.array_equal(match[:, d, d, 1], counts[:, :, 3])
    assert counts[:, 1:, 2].any()


def test_diagonal_equals_clip_counts(dev):
    for content in ('shifted', 'void'):
        _equals_the_diagonal_scorer(dev, *_content((4, 64, 256), content, 10, 10), 10)


def test_diagonal_equals_clip_counts_at_480p(dev):
    a = census_ref.blobs(11, 1, 480, 854)
    b = np.roll(a, (5, 9), axis=(1, 2))
    b[0, 100:140, 300:420] = 255
    _equals_the_diagonal_scorer(dev, a, b, 10)


def test_side_stream_twice(dev):
    """on a non-default stream, twice in a row, the blocks the outputs get next dirtied: byte-identical, and the reference's"""
    from rmem_ocu_amd.pairs import pair_boundary_counts
    shape, nums = (2, 37, 131), (65, 70)
    a, b = _device(dev, *_content(shape, 'different', *nums))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = []
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.full((shape[0] * (nums[0] + 1) * (nums[1] + 1) * 2,), CANARY32, dtype=torch.int32, device=dev)
            got.append(pair_boundary_counts(a, b, *nums, bound_th=2))
        side.synchronize()
    want = _ref(shape, 'different', *nums, 255, 2)
    for x, y, w in zip(got[0], got[1], want):
        assert x.dtype == torch.int32 and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert np.array_equal(x.cpu().numpy(), w)


def test_python_interface_on_the_device(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd import pairs
    x = torch.zeros(2, 4, 4, dtype=torch.uint8, device=dev)
    with pytest.raises(RmemError, match='one shape'):
        pairs.pair_boundary_counts(x, x[:1], 3, 3)
    with pytest.raises(RmemError, match='device tensor'):
        pairs.pair_boundary_counts(x, x.cpu(), 3, 3)
    with pytest.raises(RmemError, match='device tensor'):
        pairs.pair_boundary_counts(x, x.int(), 3, 3)
    with pytest.raises(RmemError, match='workspace_bytes'):
        pairs.pair_boundary_counts(x, x, 3, 3, workspace_bytes=8 * 4 * 8 - 1)
    with pytest.raises(RmemError, match='radius'):
        pairs.pair_boundary_counts(x, x, 3, 3, bound_th=64)
    a, b = _content((3, 17, 33), 'void', 5, 3)
    ad, bd = _device(dev, a, b)
    want = _ref((3, 17, 33), 'void', 5, 3, 255, 2)
    per_frame = 10 * 17 * 8
    for kw in (dict(), dict(workspace_bytes=per_frame), dict(workspace_bytes=2 * per_frame + 5)):
        got = pairs.pair_boundary_counts(ad, bd, 5, 3, bound_th=2, **kw)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    one = pairs.pair_boundary_counts(ad[0], bd[0], 5, 3, bound_th=2)          # [H, W] is one frame
    assert tuple(one[0].shape) == (1, 6, 4, 2) and np.array_equal(one[0].cpu().numpy()[0], want[0][0])
    J, F = pairs.pair_jf(ad, bd, 5, 3, bound_th=2)
    assert np.array_equal(F, ref.f_table(*want))
    other = b > 3                                                   # J: annotated values above num_b, void among them, count nowhere
    for f, i, j in ((0, 1, 1), (1, 2, 3), (2, 5, 2), (2, 4, 1)):
        A, B = (a[f] == i) & ~other[f], (b[f] == j) & ~other[f]
        assert J[f, i - 1, j - 1] == boundary_ref.j_from_counts(int((A & B).sum()), int((A | B).sum()))


# ------------------------------------------------------------------------------------------------------------ the evaluator
def _clip(n, H, W, num, void=True):
    """annotations with `num` boxes on a grid that drift one pixel down per frame, and a prediction: the annotation moved by
    (1, 2) pixels with object 2 lost from frame 3 on"""
    gt = np.zeros((n, H, W), dtype=np.uint8)
    cols = int(np.ceil(np.sqrt(num)))
    ch, cw = (H - n) // -(-num // cols), W // cols
    for v in range(1, num + 1):
        y, x = ((v - 1) // cols) * ch, ((v - 1) % cols) * cw
        for f in range(n):
            gt[f, y + 1 + f:y + ch - 1 + f - v % 2, x + 1:x + cw - 1 - v % 3] = v
    pred = np.roll(gt, (1, 2), axis=(1, 2))
    pred[3:][pred[3:] == 2] = 0
    if void:
        gt[:, 0, W - 9:] = 255
        gt[2, H // 2:H // 2 + 3, :W // 2] = 255
    return pred, gt


def _same_score(x, y):
    for f in dataclasses.fields(x):
        u, v = getattr(x, f.name), getattr(y, f.name)
        if f.name == 'obj_frames':
            assert u is None and v is None
        else:
            assert np.array_equal(np.asarray(u), np.asarray(v)), f.name


def test_score_clip_objects_equals_score_clip(dev):
    from rmem_ocu_amd.evaluator import score_clip, score_clip_objects
    pred, gt = _clip(6, 48, 80, 10)
    assert all((pred == v).any() and (gt == v).any() for v in range(1, 11))
    p, g = _device(dev, pred, gt)
    for kw in (dict(), dict(num_objs=10), dict(frames=slice(0, None), tail=0.5), dict(bound_th=2)):
        _same_score(score_clip_objects(p, g, **kw), score_clip(p, g, **kw))
    # fewer objects than the stacks hold: predicted values above num_objs are no objects on either route (annotated ones that are
    # not void differ by design, see score_clip_objects)
    g7 = _device(dev, np.where((gt > 7) & (gt != 255), 0, gt).astype(np.uint8))[0]
    _same_score(score_clip_objects(p, g7, 7), score_clip(p, g7, 7))


def test_score_clip_objects_beyond_31_objects(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import score_clip, score_clip_objects
    n, num = 5, 40
    pred, gt = _clip(n, 69, 112, num)
    assert all((gt == v).any() for v in range(1, num + 1))
    p, g = _device(dev, pred, gt)
    with pytest.raises(RmemError, match=r'1\.\.31'):
        score_clip(p, g, num)
    got = score_clip_objects(p, g)
    match, bnd_a, bnd_b = ref.tables(pred, gt, num, num, 255, 0.008)
    counts = np.zeros((n, num + 1, 6), dtype=np.int64)
    d = np.arange(num + 1)
    counts[..., 0], counts[..., 1], counts[..., 2], counts[..., 3] = bnd_a, bnd_b, match[:, d, d, 0], match[:, d, d, 1]
    void = gt == 255
    for k in range(1, num + 1):
        A, B = (pred == k) & ~void, (gt == k) & ~void
        counts[:, k, 4], counts[:, k, 5] = (A & B).sum(axis=(1, 2)), (A | B).sum(axis=(1, 2))
    Jr, Fr = boundary_ref.scores(counts)
    assert got.J.shape == (n, num) and np.array_equal(got.J, Jr[:, 1:]) and np.array_equal(got.F, Fr[:, 1:])
    # the summary is float64 sums of a few dozen values in [0, 1] by two codes: they agree to rounding, test_hip_boundary's bound
    for name, v in boundary_ref.summary(Jr[:, 1:], Fr[:, 1:]).items():
        assert np.abs(np.asarray(getattr(got, name)) - np.asarray(v)).max() < 1e-12, name
    assert 0.0 < got.F_mean < 1.0 and 0.0 < got.J_mean < 1.0


def test_score_unsupervised_clip(dev):
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import score_clip, score_unsupervised_clip
    pred, gt = _clip(6, 48, 80, 4)
    perm = np.arange(256, dtype=np.uint8)
    perm[[1, 2, 3, 4]] = [3, 1, 4, 2]                               # the proposal that follows annotated object 1 is called 3, ...
    mixed = perm[pred]
    p, g, m = _device(dev, pred, gt, mixed)
    want = score_clip(p, g, 4, frames=slice(None))
    got, mapping = score_unsupervised_clip(m, g, 4)
    assert mapping == {1: 3, 2: 1, 3: 4, 4: 2}
    _same_score(got, want)
    got, mapping = score_unsupervised_clip(m, g, 4, 4)
    assert mapping == {1: 3, 2: 1, 3: 4, 4: 2}
    _same_score(got, want)
    # proposal 4 (annotated object 3) removed: the orphan scores against an empty prediction
    fewer = np.where(mixed == 4, 0, mixed).astype(np.uint8)
    got, mapping = score_unsupervised_clip(_device(dev, fewer)[0], g, 3)
    assert mapping == {1: 3, 2: 1, 3: None, 4: 2}
    empty = score_clip(_device(dev, np.where(pred == 3, 0, pred).astype(np.uint8))[0], g, 4, frames=slice(None))
    _same_score(got, empty)
    assert not got.J[:, 2].any() and not got.F[:, 2].any()
    # an extra proposal that overlaps nothing annotated changes nothing
    extra = mixed.copy()
    assert not extra[:, 0, :20].any() and not gt[:, 0, :20].any()
    extra[:, 0, :20] = 5
    got, mapping = score_unsupervised_clip(_device(dev, extra)[0], g, 5)
    assert mapping == {1: 3, 2: 1, 3: 4, 4: 2}
    _same_score(got, want)
    with pytest.raises(RmemError, match='max_proposals'):
        score_unsupervised_clip(m, g, 4, max_proposals=3)
