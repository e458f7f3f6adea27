"""COCO run-length masks on the MI355X against tests/rle_ref.py: byte and integer equality everywhere.  Labels between guard
bytes at several byte offsets, outputs pre-filled with 0xA5 and followed by guards, workspaces handed over dirty."""
import functools

import numpy as np
import pytest
import torch

import census_ref
import rle_ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
CANARY64 = int(np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0])
FULL = (1, 480, 854)
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (3, 5, 33), (2, 37, 131), (4, 64, 256), (2, 130, 300), FULL]
CONTENTS = ['zero', 'one id', 'random', 'blobs', 'corners', 'vstripes', 'hstripes', 'checker', 'above']
CASES = [(s, c) for s in SHAPES for c in CONTENTS if s != FULL or c == 'blobs']
IDS = [f'{"x".join(map(str, s))}-{c}' for s, c in CASES]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _stack(shape, content, K):
    """the label stack of one (shape, content, num_ids): computed once, shared, read only"""
    n, H, W = shape
    rng = np.random.default_rng(n * 7919 + H * 131 + W + K)
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'zero':
        a = np.zeros(shape, dtype=np.uint8)
    elif content == 'one id':
        a = np.full(shape, K, dtype=np.uint8)
    elif content == 'random':
        a = rng.integers(0, K + 1, shape).astype(np.uint8)
    elif content == 'blobs':                                            # ids 1..10: with K = 1 nine of them belong to no mask
        a = census_ref.blobs(H * W + n, n, H, W)
    elif content == 'corners':
        a = np.zeros(shape, dtype=np.uint8)
        for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            a[:, y, x] = min(K, i + 1)
    elif content == 'vstripes':
        a = np.broadcast_to((xx % min(K + 1, 4)).astype(np.uint8), shape).copy()
    elif content == 'hstripes':                                         # a boundary at every pixel
        a = np.broadcast_to((yy % min(K, 3) + 1).astype(np.uint8) if H > 1 else (xx % 2).astype(np.uint8), shape).copy()
    elif content == 'checker':
        a = np.broadcast_to((((yy + xx) % 2) * K).astype(np.uint8), shape).copy()
    else:                                                               # values above num_ids: they belong to no mask
        a = rng.integers(0, min(K + 4, 256), shape).astype(np.uint8)
        a[:, 0, 0] = min(K + 1, 255)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(shape, content, K):
    per_frame = rle_ref.encode_labels(_stack(shape, content, K), K)
    return tuple(s for fr in per_frame for s in fr)


def _guarded(dev, a, offset, fill=None):
    """a's bytes (or `fill`) on the device between guard bytes, `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1) if fill is None else fill
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size].view(a.shape), front


def _guards_intact(buf, front, size):
    b = buf.cpu().numpy()
    return bool((b[:front] == CANARY).all() and (b[front + size:] == CANARY).all())


def _encode(dev, a, K, offset=0, capacity=None):
    """rmem_rle_encode_labels on a guarded copy of a, a dirty workspace, out / offsets / status pre-filled with 0xA5 and followed
    by guards -> (strings or None, offsets, status word, out bytes)"""
    from rmem_ocu_amd import _lib
    n, H, W = a.shape
    L = _lib.lib()
    S = n * K
    buf, view, front = _guarded(dev, a, offset)
    nbytes = L.rmem_rle_workspace_bytes(n, H, W, K)
    assert nbytes > 0
    ws = torch.full((nbytes,), CANARY, dtype=torch.uint8, device=dev)
    cap = 6 * (2 * H * W + K) * n if capacity is None else capacity
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device=dev)
    offsets = torch.full((S + 1 + 8,), CANARY64, dtype=torch.int64, device=dev)
    status = torch.full((1 + 8,), CANARY32, dtype=torch.int32, device=dev)
    _lib.check(L.rmem_rle_encode_labels(view.data_ptr(), n, H, W, K, ws.data_ptr(), out.data_ptr(), cap, offsets.data_ptr(),
                                        status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), 'rmem_rle_encode_labels')
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, a.size), 'guard bytes around the labels'
    assert np.array_equal(buf[front:front + a.size].cpu().numpy(), a.reshape(-1)), 'the labels are read only'
    off, st, o = offsets.cpu().numpy(), status.cpu().numpy(), out.cpu().numpy()
    assert (off[S + 1:] == CANARY64).all() and (st[1:] == CANARY32).all(), 'beyond offsets / status'
    off = off[:S + 1].tolist()
    used = off[S] if off[S] <= cap else 0
    assert (o[used:] == CANARY).all(), 'bytes of out beyond the strings were written'
    strings = None if off[S] > cap else [o[p:q].tobytes() for p, q in zip(off, off[1:])]
    return strings, off, int(st[0]), o[:cap]


def _check_encode(dev, shape, content, K, offsets):
    a, want = _stack(shape, content, K), _ref(shape, content, K)
    want_off = np.concatenate(([0], np.cumsum([len(s) for s in want]))).tolist()
    for offset in offsets:
        got, off, st, _ = _encode(dev, a, K, offset)
        assert st == 0 and off == want_off, (offset, off[:8], want_off[:8])
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (offset, bad[:4], got[bad[0]][:40], want[bad[0]][:40])


@pytest.mark.parametrize('shape,content', CASES, ids=IDS)
def test_encode(dev, shape, content):
    """every string and every offset equals the reference's, for num_ids 1 and 10, labels at byte offsets 0, 1, 3, 13"""
    for K in (1, 10):
        _check_encode(dev, shape, content, K, (0, 13) if shape == FULL else (0, 1, 3, 13))


@pytest.mark.parametrize('content', ['random', 'above', 'hstripes'])
def test_encode_255_ids(dev, content):
    a = _stack((2, 37, 131), content, 255)
    if content != 'hstripes':
        assert len(np.unique(a)) == 256
    _check_encode(dev, (2, 37, 131), content, 255, (0, 3))


def test_six_character_count(dev):
    """4096 x 4100 (H * W > 2^24), all zero but the last pixel: the only way to the sixth character of a count, both directions"""
    from rmem_ocu_amd import rle
    H, W = 4096, 4100
    a = np.zeros((1, H, W), dtype=np.uint8)
    a[0, H - 1, W - 1] = 1
    want = rle_ref.to_string(rle_ref.counts_of(a[0]))
    assert len(want) == 7 and rle_ref.from_string(want) == [H * W - 1, 1]
    t = torch.from_numpy(a).to(dev)
    out, offsets, status = rle.encode(t, 1, 64)
    torch.cuda.synchronize()
    assert status.item() == 0 and offsets.tolist() == [0, 7] and out[:7].cpu().numpy().tobytes() == want
    back = rle.decode_label_stack([{1: {'size': [H, W], 'counts': want}}], (H, W), dev)
    assert torch.equal(back, t)


@pytest.mark.parametrize('shape,content,K', [((3, 5, 33), 'random', 10), ((2, 37, 131), 'blobs', 10), ((1, 1, 1), 'zero', 1)])
def test_capacity(dev, shape, content, K):
    """one byte short: the capacity bit, exact offsets, no byte of out changed"""
    a, want = _stack(shape, content, K), _ref(shape, content, K)
    total = sum(len(s) for s in want)
    got, off, st, o = _encode(dev, a, K, 1, capacity=total - 1)
    from rmem_ocu_amd import rle
    assert got is None and st == rle.ST_CAPACITY
    assert off == np.concatenate(([0], np.cumsum([len(s) for s in want]))).tolist()
    assert (o == CANARY).all()
    got, off, st, _ = _encode(dev, a, K, 1, capacity=total)                 # exactly enough
    assert st == 0 and got == list(want)


def test_encode_label_stack_retries_with_the_exact_size(dev, monkeypatch):
    from rmem_ocu_amd import rle
    shape, K = (4, 64, 256), 10
    a, want = _stack(shape, 'random', K), _ref(shape, 'random', K)
    t = torch.from_numpy(a.copy()).to(dev)
    generous = rle.encode_label_stack(t, K)
    monkeypatch.setattr(rle, 'default_capacity', lambda n, H, W, k: 1)
    tiny = rle.encode_label_stack(t, K)
    monkeypatch.setattr(rle, 'frames_per_call', lambda H, W, k: 3)          # chunks of 3 and 1 frames
    chunked = rle.encode_label_stack(t, K, ascii=True)
    assert generous == tiny
    assert [[fr[k]['counts'] for k in range(1, K + 1)] for fr in generous] == [list(want[f * K:(f + 1) * K]) for f in range(shape[0])]
    assert all(fr[k]['size'] == [64, 256] for fr in generous for k in fr)
    assert [[fr[k]['counts'].encode() for k in range(1, K + 1)] for fr in chunked] == [[fr[k]['counts'] for k in range(1, K + 1)] for fr in tiny]


def _decode(dev, frames, shape, offset=0):
    """rle.decode_labels_into on a guarded, 0xA5-filled stack and a dirty workspace -> (uint8 [n, H, W], PackedRles)"""
    from rmem_ocu_amd import _codec, _lib, rle
    n, H, W = shape
    packed = frames if isinstance(frames, rle.PackedRles) else rle.PackedRles(frames, (H, W))
    blank = np.zeros(shape, dtype=np.uint8)
    buf, view, front = _guarded(dev, blank, offset, fill=CANARY)
    nbytes = _lib.lib().rmem_rle_decode_workspace_bytes(len(packed), packed.total_bytes, n, W)
    assert nbytes > 0
    _codec.workspace('rle.decode', dev, None, nbytes).fill_(CANARY)
    rle.decode_labels_into(packed, view)
    torch.cuda.synchronize()
    assert _guards_intact(buf, front, blank.size), 'guard bytes around the decoded stack'
    return view.cpu().numpy(), packed


@pytest.mark.parametrize('shape,content', CASES, ids=IDS)
def test_decode(dev, shape, content):
    """the reference's strings decode to the label stack (values above num_ids zeroed), reassembled from the per-id masks"""
    n, H, W = shape
    for K, offset in ((1, 0), (10, 3)):
        a, strings = _stack(shape, content, K), _ref(shape, content, K)
        frames = [[(k, {'size': [H, W], 'counts': strings[f * K + k - 1]}) for k in range(1, K + 1)] for f in range(n)]
        got, packed = _decode(dev, frames, shape, offset)
        assert packed.status(dev).cpu().tolist() == [0] * (n * K)
        assert np.array_equal(got, np.where(a > K, 0, a)), (K, np.argwhere(got != np.where(a > K, 0, a))[:4])


def test_decode_255_ids(dev):
    shape, K = (2, 37, 131), 255
    a, strings = _stack(shape, 'random', K), _ref(shape, 'random', K)
    frames = [{k: {'size': [37, 131], 'counts': strings[f * K + k - 1].decode()} for k in range(1, K + 1)} for f in range(2)]
    got, packed = _decode(dev, frames, shape)
    packed.check(dev)
    assert np.array_equal(got, a)


def test_decode_overlap_and_list_counts(dev):
    """two overlapping boxes in both orders: the later one wins; uncompressed list counts give the same stack; a frame without
    masks is zero"""
    H, W = 37, 131
    m1, m2 = np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
    m1[3:20, 10:70] = 1
    m2[12:30, 40:120] = 1
    c1, c2 = rle_ref.counts_of(m1), rle_ref.counts_of(m2)
    s1, s2 = ({'size': [H, W], 'counts': rle_ref.to_string(c)} for c in (c1, c2))
    l1, l2 = ({'size': [H, W], 'counts': c} for c in (c1, c2))
    frames = [[(7, s1), (9, s2)], [], [(9, s2), (7, s1)], [(7, l1), (9, l2)]]
    want = rle_ref.paint([[(7, c1), (9, c2)], [], [(9, c2), (7, c1)], [(7, c1), (9, c2)]], H, W)
    assert want[0, 15, 50] == 9 and want[2, 15, 50] == 7 and not want[1].any()
    got, packed = _decode(dev, frames, (4, H, W), 1)
    packed.check(dev)
    assert np.array_equal(got, want)


def test_malformed_strings(dev):
    """one string per status bit: each sets exactly its bit, paints nothing, and nothing is touched out of range"""
    from rmem_ocu_amd import rle
    from rmem_ocu_amd._lib import RmemError
    H, W = 6, 5                                                             # H * W = 30
    mA, mB = np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
    mA[1:4, 1:3] = 1
    mB[0:6, 4] = 1
    cA, cB = rle_ref.counts_of(mA), rle_ref.counts_of(mB)
    good_a, good_b = rle_ref.to_string(cA), rle_ref.to_string(cB)
    full = rle_ref.to_string([0, 30])                                       # would paint the whole frame if it were taken
    assert rle_ref.to_string([30]) == b'n0'

    def r(counts):
        return {'size': [H, W], 'counts': counts}

    listing = [
        (0, 2, r(good_a), 0),
        (0, 3, r(b'/' + full[1:]), rle.ST_CHAR),                            # 47
        (0, 3, r(full[:1] + b'p'), rle.ST_CHAR),                            # 112
        (0, 3, r(b'0n'), rle.ST_TRUNCATED),                                 # [0, 30] cut inside its second count
        (0, 3, r(b'0' + bytes([48 + 0x20 + 30]) + bytes([48 + 0x20]) * 5 + b'0'), rle.ST_LONG),   # 30 written with seven characters
        (1, 5, r(rle.string_from_counts([10, -2, 22])), rle.ST_NEGATIVE),
        (1, 5, r([0, 31]), rle.ST_SUM),
        (1, 5, r([0, 29]), rle.ST_SUM),
        (1, 4, r(good_b), 0),
        (1, 6, r(full), rle.ST_DESC),                                       # its descriptor is given frame = frames below
    ]
    frames = [[(v, e) for f, v, e, _ in listing if f == k] for k in range(2)]
    packed = rle.PackedRles(frames, (H, W))
    assert len(packed) == len(listing)
    packed.descs[len(listing) - 1].frame = 2
    packed.desc_bytes = torch.frombuffer(bytearray(packed.descs), dtype=torch.uint8).pin_memory()
    got, packed = _decode(dev, packed, (2, H, W), 1)
    assert packed.status(dev).cpu().tolist() == [st for _, _, _, st in listing]
    assert np.array_equal(got, rle_ref.paint([[(2, cA)], [(4, cB)]], H, W))
    with pytest.raises(RmemError, match=r'status 1: a byte outside 48\.\.111\); 8 frames bad \[string 1: frame 0, value 3\]'):
        packed.check(dev)
    packed.check(dev, 0, 1)
    with pytest.raises(RmemError, match=r'status 32: bad descriptor\) \[string 9: frame 1, value 6\]'):
        packed.check(dev, 8)
    with pytest.raises(RmemError, match='string 1'):
        rle.decode_label_stack(frames, (H, W), dev)


def test_bad_descriptor_ranges(dev):
    """ranges outside bits, a value of 0, a frame below the one before: ST_DESC each, the rest still decodes"""
    from rmem_ocu_amd import rle
    H, W = 6, 5
    m = np.zeros((H, W), dtype=np.uint8)
    m[2:5, 0:2] = 1
    c = rle_ref.counts_of(m)
    e = {'size': [H, W], 'counts': rle_ref.to_string(c)}
    packed = rle.PackedRles([[(1, e), (2, e)], [(3, e), (4, e), (5, e)]], (H, W))
    packed.descs[1].offset = packed.total_bytes - 1                         # runs past the end of bits
    packed.descs[2].value = 0
    packed.descs[3].offset = -1
    packed.descs[4].frame = 0                                               # below the frame of the string before
    packed.desc_bytes = torch.frombuffer(bytearray(packed.descs), dtype=torch.uint8).pin_memory()
    got, packed = _decode(dev, packed, (2, H, W))
    assert packed.status(dev).cpu().tolist() == [0, rle.ST_DESC, rle.ST_DESC, rle.ST_DESC, rle.ST_DESC]
    assert np.array_equal(got, rle_ref.paint([[(1, c)], []], H, W))


def test_round_trip_on_a_side_stream(dev):
    """labels_from_rles(rle_results(stack)) is the stack with values above K zeroed: on a non-default stream, after both
    workspaces were dirtied there, twice in a row with identical bytes"""
    from rmem_ocu_amd import _codec, _lib, rle
    from rmem_ocu_amd.evaluator import labels_from_rles, rle_results
    shape, K = (4, 64, 256), 7
    a = _stack(shape, 'blobs', 10)
    t = torch.from_numpy(a.copy()).to(dev)
    want = torch.from_numpy(np.where(a > K, 0, a)).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    results = []
    with torch.cuda.stream(side):
        for _ in range(2):
            _codec.workspace('rle.encode', dev, side, _lib.lib().rmem_rle_workspace_bytes(*shape, K)).fill_(CANARY)
            _codec.workspace('rle.decode', dev, side, 1 << 20).fill_(CANARY)
            res = rle_results(t, K, ascii=True)
            assert all(isinstance(fr[k]['counts'], str) for fr in res for k in fr) and [sorted(fr) for fr in res] == [list(range(1, K + 1))] * 4
            back, ids = labels_from_rles(res, shape[1:], dev)
            side.synchronize()
            assert ids == list(range(1, K + 1)) and torch.equal(back, want)
            results.append(res)
    assert results[0] == results[1]
    assert [[fr[k]['counts'].encode() for k in range(1, K + 1)] for fr in results[0]] == [list(r) for r in rle_ref.encode_labels(a, K)]


def _annotations():
    """[6, 37, 131]: tracks 3 and 7 on frame 0, 200 enters on frame 4 (and 7 is hidden on frame 2)"""
    a = np.zeros((6, 37, 131), dtype=np.uint8)
    for f in range(6):
        a[f, 2 + f:12 + f, 5:40] = 7
        a[f, 20:30, 60 + 3 * f:100 + 3 * f] = 3
    a[2][a[2] == 7] = 0
    for f in (4, 5):
        a[f, 8:19, 90 + f:117 + f] = 200
    return a


def test_protocol_plumbing(dev):
    """annotations delivered as run-length tracks give the clip protocol the same objects, first frames, first label and
    overlays as the same annotations delivered as palette PNGs"""
    from rmem_ocu_amd import png
    from rmem_ocu_amd.evaluator import labels_from_pngs, labels_from_rles
    from rmem_ocu_amd.protocol import clip_protocol
    a = _annotations()
    tracks = [{int(v): {'size': [37, 131], 'counts': rle_ref.to_string(rle_ref.counts_of(fr == v)).decode()} for v in np.unique(fr) if v}
              for fr in a]
    stack, ids = labels_from_rles(tracks, (37, 131), dev)
    assert ids == [3, 7, 200] and stack.dtype == torch.uint8 and tuple(stack.shape) == a.shape
    lut = np.zeros(256, dtype=np.uint8)
    lut[[3, 7, 200]] = [1, 2, 3]
    assert np.array_equal(stack.cpu().numpy(), lut[a])
    from_png = labels_from_pngs(png.encode_label_stack(torch.from_numpy(a).to(dev)), dev)
    p_rle, first_rle, new_rle = clip_protocol(stack)
    p_png, first_png, new_png = clip_protocol(from_png)
    assert p_png.squeeze_idx == [0, 3, 7, 200]
    assert [0] + [ids[v - 1] for v in p_rle.squeeze_idx[1:]] == p_png.squeeze_idx
    assert p_rle.first_frame.tolist() == p_png.first_frame.tolist() == [0, 0, 4] and p_rle.new_frames == p_png.new_frames == [4]
    assert torch.equal(first_rle, first_png) and sorted(new_rle) == sorted(new_png) == [4] and torch.equal(new_rle[4], new_png[4])
    sub, sub_ids = labels_from_rles(tracks, (37, 131), dev, ids=[200, 7])   # chosen ids: the others are left out
    want = np.zeros(256, dtype=np.uint8)
    want[[200, 7]] = [1, 2]
    assert sub_ids == [200, 7] and np.array_equal(sub.cpu().numpy(), want[a])


def test_boxes(dev):
    """area = the sum of the odd-indexed counts, bbox = the numpy box of the mask, keys through squeeze_idx"""
    from rmem_ocu_amd.evaluator import rle_results
    a = census_ref.blobs(5, 3, 64, 96, ids=(1, 2, 3, 4, 5, 9))
    a[1][a[1] == 3] = 0                                                     # object 3 is absent from frame 1
    squeeze_idx = [0, 11, 22, 33, 44, 55]
    res = rle_results(torch.from_numpy(a).to(dev), 6, squeeze_idx, boxes=True, ascii=False)
    assert [sorted(fr) for fr in res] == [[11, 22, 33, 44, 55]] * 3          # id 6 is beyond squeeze_idx
    seen = 0
    for f, fr in enumerate(res):
        for k in range(1, 6):
            e, m = fr[squeeze_idx[k]], a[f] == k
            counts = rle_ref.from_string(e['counts'])
            assert e['counts'] == rle_ref.to_string(rle_ref.counts_of(m)) and e['area'] == sum(counts[1::2]) == int(m.sum())
            if m.any():
                ys, xs = np.nonzero(m)
                assert e['bbox'] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
                seen += 1
            else:
                assert e['bbox'] == [0, 0, 0, 0] and e['area'] == 0
    assert seen >= 5 and res[1][33]['area'] == 0
