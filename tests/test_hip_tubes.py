"""Label tubes on the MI355X against tests/tubes_ref.py (scipy.ndimage.label on the 3-D structures): exact integer equality of
tubes, links, events, rank, total, table and the cleaned stacks, and a status word of 0, in every case.  The stack sits between
guard bytes and starts at any byte, every output is dirtied first and followed by guard words, the shapes lie around the 32 x 64
tile of the 2-D kernels and around n = 1, 2.  Content and references are computed once per case."""
import functools
import warnings

import numpy as np
import pytest
import torch

import tubes_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 33, 65), (2, 32, 64), (3, 5, 7), (5, 31, 127), (6, 97, 131)]
SHAPE_IDS = ['x'.join(str(k) for k in s) for s in SHAPES]
CONFIGS = [(4, 1), (4, 9), (8, 1), (8, 9)]
FULL = (4, 480, 854)


def _rules(n):
    return [(0, 0), (2, 0), (3, 2), (n + 1, n)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _ref(shape, content, conn, temp):
    """every reference output of one case: computed once, shared, read only"""
    return R.everything(R.content(content, *shape), conn, temp)


@functools.lru_cache(maxsize=None)
def _ref_clean(shape, content, conn, temp, rule):
    ref = _ref(shape, content, conn, temp)
    out = R.clean(R.content(content, *shape), rule[0], rule[1], conn, temp, ref['roots'], ref['stats'], ref['tubes'], ref['table'])
    out.setflags(write=False)
    return out


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


def _dirty(dev, size):
    return torch.full((size + 64,), CANARY32, dtype=torch.int32, device=dev)


def _take(t, size, shape):
    h = t.cpu().numpy()
    assert (h[size:] == CANARY32).all(), 'words beyond an output were written'
    return h[:size].reshape(shape)


def _run(dev, a, conn, temp, offset=0, stream=None, rows=None, rules=()):
    """every entry point on a guarded copy of a -> dict of numpy outputs; outputs dirtied and guarded, status 0.  rows: None takes
    the table whole (total rows).  rules: the cleaned stack of every (min_frames, max_hole_frames), out of place."""
    from rmem_ocu_amd import _lib
    n, H, W = a.shape
    N, HW = a.size, H * W
    L = _lib.lib()
    ts = torch.cuda.current_stream(dev) if stream is None else stream
    s = ts.cuda_stream
    with torch.cuda.stream(ts):
        buf, view, front = _guarded(dev, a, offset)
        roots, stats, ctable = _dirty(dev, N), _dirty(dev, N * 4), _dirty(dev, n * 768)
        tubes, links, events, rank, total = _dirty(dev, N), _dirty(dev, N * 4), _dirty(dev, n * 1024), _dirty(dev, N), _dirty(dev, 1)
        status = _dirty(dev, 1)
        status[0] = 0
        p = view.data_ptr()
        _lib.check(L.rmem_label_components(p, n, H, W, conn, roots.data_ptr(), status.data_ptr(), s), 'rmem_label_components')
        _lib.check(L.rmem_label_component_stats(p, roots.data_ptr(), n, H, W, conn, stats.data_ptr(), ctable.data_ptr(), s),
                   'rmem_label_component_stats')
        _lib.check(L.rmem_label_tubes(p, roots.data_ptr(), n, H, W, temp, tubes.data_ptr(), status.data_ptr(), s), 'rmem_label_tubes')
        _lib.check(L.rmem_label_tube_lineage(p, roots.data_ptr(), n, H, W, temp, links.data_ptr(), s), 'rmem_label_tube_lineage')
        _lib.check(L.rmem_label_tube_events(p, roots.data_ptr(), links.data_ptr(), n, H, W, events.data_ptr(), s), 'rmem_label_tube_events')
        _lib.check(L.rmem_label_tube_index(tubes.data_ptr(), n, H, W, rank.data_ptr(), total.data_ptr(), s), 'rmem_label_tube_index')
        ts.synchronize()
        T = int(_take(total, 1, (1,))[0])
        assert 1 <= T <= N
        k = T if rows is None else rows
        table = _dirty(dev, k * 10)
        _lib.check(L.rmem_label_tube_table(p, roots.data_ptr(), stats.data_ptr(), tubes.data_ptr(), rank.data_ptr(), n, H, W, k,
                                           table.data_ptr(), s), 'rmem_label_tube_table')
        cleaned = []
        if rows is None:
            for life, hole in rules:
                dbuf, dview, dfront = _guarded(dev, np.full(a.shape, CANARY, dtype=np.uint8), offset)
                _lib.check(L.rmem_label_tube_clean(p, dview.data_ptr(), roots.data_ptr(), stats.data_ptr(), tubes.data_ptr(), rank.data_ptr(),
                                                   table.data_ptr(), n, H, W, life, hole, s), 'rmem_label_tube_clean')
                cleaned.append((dbuf, dview, dfront))
        ts.synchronize()
        assert _guards_intact(buf, front, N), 'guard bytes around the stack'
        assert np.array_equal(view.cpu().numpy(), a), 'the stack is read only'
        assert int(_take(status, 1, (1,))[0]) == 0, 'status'
        out = dict(roots=_take(roots, N, a.shape), stats=_take(stats, N * 4, (n, HW, 4)), tubes=_take(tubes, N, a.shape),
                   links=_take(links, N * 4, (n, HW, 4)), events=_take(events, n * 1024, (n, 256, 4)), rank=_take(rank, N, a.shape), total=T,
                   table=_take(table, k * 10, (k, 10)), clean=[])
        for dbuf, dview, dfront in cleaned:
            assert _guards_intact(dbuf, dfront, N), 'guard bytes around the cleaned stack'
            out['clean'].append(dview.cpu().numpy())
    return out


def _compare(got, ref, where):
    for key in ('roots', 'stats', 'tubes', 'links', 'events', 'rank', 'table'):
        assert np.array_equal(got[key], ref[key]), (key, where, np.argwhere(got[key] != ref[key])[:8])
    assert got['total'] == ref['total'], where


@pytest.mark.parametrize('content', R.CONTENTS)
@pytest.mark.parametrize('k', range(len(SHAPES)), ids=SHAPE_IDS)
def test_tubes_lineage_events_index_table_and_clean(dev, k, content):
    """every output as a whole array, both connectivities, both temporal reaches, the stack starting at every byte offset"""
    shape = SHAPES[k]
    a = R.content(content, *shape)
    rules = _rules(shape[0])
    for conn, temp in CONFIGS:
        ref = _ref(shape, content, conn, temp)
        for offset in OFFSETS:
            got = _run(dev, a, conn, temp, offset, rules=rules)
            _compare(got, ref, (content, conn, temp, offset))
            for rule, cleaned in zip(rules, got['clean']):
                want = _ref_clean(shape, content, conn, temp, rule)
                assert np.array_equal(cleaned, want), (content, conn, temp, offset, rule, np.argwhere(cleaned != want)[:8])
                if rule == (0, 0):
                    assert np.array_equal(want, a), 'the identity'


def test_contents_are_what_they_claim():
    """by the reference alone: the inverted checkerboard links nothing under (4, 1), the staircase is one tube through all frames,
    and the clean rules change something somewhere"""
    n, H, W = shape = SHAPES[-1]
    assert _ref(shape, 'flip', 4, 1)['total'] == n * H * W
    assert _ref(shape, 'checker', 4, 1)['total'] == H * W and _ref(shape, 'checker', 8, 1)['total'] == 2
    stairs, runs = _ref(shape, 'stairs', 8, 1)['table'], R.content('stairs', *shape).sum(axis=(1, 2))
    assert stairs[stairs[:, 1] == 1].tolist() == [[0, 1, int(runs.sum()), n, 0, n - 1, 0, 0, 1, int(runs.max())]]
    assert not np.array_equal(_ref_clean(shape, 'drift', 8, 1, (3, 2)), R.content('drift', *shape))
    assert not np.array_equal(_ref_clean(shape, 'noise', 8, 1, (n + 1, n)), R.content('noise', *shape))


@pytest.mark.parametrize('content', ['drift', 'noise', 'one', 'bars'])
def test_a_table_that_is_too_small_is_cut_short(dev, content):
    """rows = total - 1: the rows before the cut are right, the words behind them untouched (rows = 0 for a stack of one tube)"""
    for shape in (SHAPES[4], SHAPES[5]):
        a = R.content(content, *shape)
        ref = _ref(shape, content, 8, 1)
        got = _run(dev, a, 8, 1, rows=ref['total'] - 1)
        assert got['total'] == ref['total'] and np.array_equal(got['table'], ref['table'][:-1]), (content, shape)


def test_clean_in_place(dev):
    """dst == src at every byte offset equals out of place"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    for shape in (SHAPES[4], SHAPES[6]):
        n, H, W = shape
        for content, conn, temp, rule in (('drift', 8, 1, (3, 2)), ('noise', 4, 9, (n + 1, n))):
            a = R.content(content, *shape)
            ref = _ref(shape, content, conn, temp)
            want = _ref_clean(shape, content, conn, temp, rule)
            assert not np.array_equal(want, a)
            r, S, t, k, T = (torch.from_numpy(ref[key].copy()).to(dev) for key in ('roots', 'stats', 'tubes', 'rank', 'table'))
            for offset in OFFSETS:
                buf, view, front = _guarded(dev, a, offset)
                _lib.check(L.rmem_label_tube_clean(view.data_ptr(), view.data_ptr(), r.data_ptr(), S.data_ptr(), t.data_ptr(), k.data_ptr(),
                                                   T.data_ptr(), n, H, W, rule[0], rule[1], s), 'rmem_label_tube_clean')
                torch.cuda.synchronize()
                assert _guards_intact(buf, front, a.size) and np.array_equal(view.cpu().numpy(), want), (content, shape, offset)


def test_a_side_stream_used_twice(dev):
    shape = SHAPES[6]
    side = torch.cuda.Stream(dev)
    for content in ('drift', 'stairs'):
        a = R.content(content, *shape)
        for _ in range(2):
            got = _run(dev, a, 8, 9, 3, stream=side, rules=[(3, 2)])
            _compare(got, _ref(shape, content, 8, 9), (content, 'side stream'))
            assert np.array_equal(got['clean'][0], _ref_clean(shape, content, 8, 9, (3, 2)))


def test_full_size_stack(dev):
    a = R.content('drift', *FULL)
    for conn, temp in ((8, 1), (4, 9)):
        got = _run(dev, a, conn, temp, 13, rules=[(3, 2)])
        _compare(got, _ref(FULL, 'drift', conn, temp), ('full size', conn, temp))
        assert np.array_equal(got['clean'][0], _ref_clean(FULL, 'drift', conn, temp, (3, 2)))


def test_index_above_the_chunk_threshold(dev):
    """above 2^26 voxels a thread of the count and rank passes takes more than 16 voxels (17 here, 16,384 chunks): ranks and total
    of a seeded set of ids against a cumulative sum on the device"""
    from rmem_ocu_amd import _lib
    n, H, W = 17, 1024, 4096
    N = n * H * W
    assert N > (1 << 26) + 4096
    g = torch.arange(N, dtype=torch.int64, device=dev)
    is_id = (((g * 2654435761) & 0xffffffff) >> 29) == 0           # one voxel in eight, voxel 0 among them
    ids = torch.where(is_id, g, torch.zeros_like(g)).to(torch.int32)
    want = torch.where(is_id, torch.cumsum(is_id, 0) - 1, torch.full_like(g, -1)).to(torch.int32)
    count = int(is_id.sum().item())
    del g
    rank, total = _dirty(dev, N), _dirty(dev, 1)
    _lib.check(_lib.lib().rmem_label_tube_index(ids.data_ptr(), n, H, W, rank.data_ptr(), total.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), 'rmem_label_tube_index')
    torch.cuda.synchronize()
    assert int(total[0].item()) == count and bool((total[1:] == CANARY32).all()) and bool((rank[N:] == CANARY32).all())
    assert torch.equal(rank[:N], want)


@pytest.mark.parametrize('offset', [0, 3])
def test_clean_strides_over_a_large_stack(dev, offset):
    """24 x 480 x 854: more 16-byte chunks than the clean kernel has threads, so every lane strides.  The references are written
    out: a rectangle of 3 on the background on frames 5..6 goes at min_frames = 3 and stays at 2; a gap of 0 inside a stack of 1 on
    frames 5..6 is filled at max_hole_frames = 2 and left at 1"""
    from rmem_ocu_amd.tubes import clean_tubes
    n, H, W = 24, 480, 854
    N = n * H * W
    buf = torch.full((64 + offset + N + 64,), CANARY, dtype=torch.uint8, device=dev)
    stack = buf[64 + offset:64 + offset + N].view(n, H, W)
    out = torch.full((64 + offset + N + 64,), CANARY, dtype=torch.uint8, device=dev)
    dst = out[64 + offset:64 + offset + N].view(n, H, W)
    for ground, patch, rule_on, rule_off in ((0, 3, (3, 0), (2, 0)), (1, 0, (0, 2), (0, 1))):
        stack.fill_(ground)
        stack[5:7, 100:300, 200:701] = patch
        before = stack.clone()
        assert clean_tubes(stack, *rule_off, out=dst) is dst and torch.equal(dst, before), (ground, rule_off)
        dst.fill_(CANARY)
        clean_tubes(stack, *rule_on, out=dst)
        assert bool((dst == ground).all()) and torch.equal(stack, before), (ground, rule_on)
        assert bool((out[:64 + offset] == CANARY).all()) and bool((out[64 + offset + N:] == CANARY).all()), 'guard bytes'
        clean_tubes(stack, *rule_on, out=stack)
        assert bool((stack == ground).all()), (ground, rule_on, 'in place')
        assert bool((buf[:64 + offset] == CANARY).all()) and bool((buf[64 + offset + N:] == CANARY).all()), 'guard bytes'


def test_python_functions(dev):
    """tubes.py and the three evaluator wrappers, [H, W] as one frame"""
    from rmem_ocu_amd import tubes
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import object_events, object_tracks, remove_flicker
    shape = n, H, W = SHAPES[5]
    for content in ('drift', 'noise'):
        a = R.content(content, *shape)
        d = torch.from_numpy(a.copy()).to(dev)
        for conn, temp in CONFIGS:
            ref = _ref(shape, content, conn, temp)
            t, status = tubes.label_tubes(d, conn, temp)
            assert t.dtype == torch.int32 and t.shape == d.shape and status.dtype == torch.int32 and status.shape == (1,)
            assert int(status.item()) == 0 and np.array_equal(t.cpu().numpy(), ref['tubes'])
            links = tubes.lineage(d, conn, temp)
            assert links.dtype == torch.int32 and links.shape == (n, H * W, 4) and np.array_equal(links.cpu().numpy(), ref['links'])
            events = tubes.piece_events(d, conn, temp)
            assert events.dtype == torch.int32 and events.shape == (n, 256, 4) and np.array_equal(events.cpu().numpy(), ref['events'])
            table, t2 = tubes.tube_table(d, conn, temp)
            assert table.dtype == torch.int32 and table.shape == (ref['total'], 10) and table.is_cuda
            assert np.array_equal(table.cpu().numpy(), ref['table']) and np.array_equal(t2.cpu().numpy(), ref['tubes'])
            for rule in _rules(n):
                want = _ref_clean(shape, content, conn, temp, rule)
                got = tubes.clean_tubes(d, rule[0], rule[1], conn, temp)
                assert got.dtype == torch.uint8 and got.shape == d.shape and got.data_ptr() != d.data_ptr()
                assert np.array_equal(got.cpu().numpy(), want), (content, conn, temp, rule)
                inplace = d.clone()
                assert tubes.clean_tubes(inplace, rule[0], rule[1], conn, temp, out=inplace) is inplace
                assert np.array_equal(inplace.cpu().numpy(), want), (content, conn, temp, rule, 'in place')
            assert np.array_equal(d.cpu().numpy(), a), 'the input is read only'
            ev = object_events(d, 10, conn, temp)
            assert ev.dtype == torch.int32 and ev.shape == (n, 11, 4) and np.array_equal(ev.cpu().numpy(), ref['events'][:, :11])
            tracks = object_tracks(d, 10, conn, temp)
            assert sorted(tracks) == list(range(1, 11))
            for v in range(1, 11):
                rows = ref['table'][ref['table'][:, 1] == v]
                assert tracks[v] == [dict(first_frame=int(r[4]), last_frame=int(r[5]), voxels=int(r[2]), pieces=int(r[3]), peak_area=int(r[9]))
                                     for r in rows], (content, conn, temp, v)
        assert np.array_equal(remove_flicker(d).cpu().numpy(), _ref_clean(shape, content, 8, 1, (3, 0)))
        assert np.array_equal(remove_flicker(d, 2, 2, 4, 9).cpu().numpy(), _ref_clean(shape, content, 4, 9, (2, 2)))
        one, _ = tubes.label_tubes(d[1], 8, 1)
        assert one.shape == (1, H, W) and np.array_equal(one.cpu().numpy()[0], _ref(shape, content, 8, 1)['roots'][1])
    x = torch.zeros(2, 4, 4, dtype=torch.uint8, device=dev)
    with pytest.raises(RmemError, match='out must be a tensor of the labels\' shape'):
        tubes.clean_tubes(x, out=x[:1])
    with pytest.raises(RmemError, match='out must be a contiguous uint8 tensor'):
        tubes.clean_tubes(x, out=x.int())
    with pytest.raises(RmemError, match='status must be an int32 tensor'):
        tubes.clean_tubes(x, status=torch.zeros(1, dtype=torch.int32))


def test_clean_tubes_with_a_status_tensor_makes_no_host_sync(dev, monkeypatch):
    """with the caller's status word nothing in clean_tubes waits for the device: every synchronising call raises meanwhile"""
    from rmem_ocu_amd.tubes import clean_tubes
    shape = SHAPES[5]
    d = torch.from_numpy(R.content('drift', *shape).copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty_like(d)
    clean_tubes(d, 3, 2, out=out, status=status)                    # the allocator holds every block now
    torch.cuda.synchronize()
    out.fill_(CANARY)

    def refuse(*a, **k):
        raise AssertionError('a host synchronisation inside clean_tubes')

    with monkeypatch.context() as m:
        for owner, name in ((torch.Tensor, 'item'), (torch.Tensor, 'cpu'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'),
                            (torch.Tensor, '__bool__'), (torch.Tensor, '__int__'), (torch.cuda, 'synchronize'),
                            (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
            m.setattr(owner, name, refuse)
        with pytest.raises(AssertionError, match='host synchronisation'):       # the check bites: status=None reads the words back
            clean_tubes(d, 3, 2, out=out)
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                         # "a prototype feature": it may miss a sync, the patches above do not
            torch.cuda.set_sync_debug_mode('error')
        try:
            got = clean_tubes(d, 3, 2, out=out, status=status)
        finally:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert got is out and int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy(), _ref_clean(shape, 'drift', 8, 1, (3, 2)))
