"""Ragged clip groups on the MI355X: the label-routing kernel (rmem_route_labels) against numpy, and clip_runner.RaggedGroupSlot --
clips of different lengths moving through the rows of one GroupEngine -- against the per-clip engines, clip by clip: label
agreement >= 0.995 per clip and identical bank traces at every frame (the bar of test_group_engine_new_object_in_one_clip and
test_hip_flip_group.py).  Geometry of the existing group tests: make_clip(seed, n, 161, 193, 2), output 160 x 192, bank 1 + 7,
gap 2 unless stated, synthetic weights."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

OUT = (160, 192)
NET = (161, 193)
OBJS = 2
CANARY = 0xA5
LENGTHS = (9, 30, 14, 22, 12)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _route_ref(rows0, table):
    """include/rmem.h, rmem_route_labels, restated: -> (rows afterwards, {row: delivered map})."""
    rows, out = rows0.copy(), {}
    for r, (has_dst, ov, fd, twin, mode) in enumerate(table):
        if mode == 2:
            continue
        if mode == 1:
            rows[r] = 0
            continue
        pred = rows0[r]
        x = fd if fd is not None else pred
        if ov is not None:
            x = np.where(ov > 0, ov, x)
        if has_dst:
            out[r] = pred if fd is not None else x
        rows[r] = x
        if twin >= 0:
            rows[twin] = x[:, ::-1]
    return rows, out


# per row: (delivers, overlay, feed, twin, mode).  Every case of the issue appears for both geometries: plain delivery, feed,
# overlay, feed + overlay, a primary with a twin, idle, live without a destination, and the twin's own skipped entry.
TABLES = {
    6: [[(1, 0, 0, -1, 0), (1, 0, 1, -1, 0), (1, 1, 0, -1, 0), (1, 1, 1, 5, 0), (0, 0, 0, -1, 1), (0, 0, 0, -1, 2)],
        [(0, 0, 0, 4, 0), (0, 1, 0, -1, 0), (1, 0, 0, -1, 0), (0, 0, 0, -1, 1), (0, 0, 0, -1, 2), (1, 0, 1, -1, 0)]],
    4: [[(1, 0, 0, 3, 0), (1, 1, 1, -1, 0), (0, 0, 0, -1, 1), (0, 0, 0, -1, 2)],
        [(0, 0, 1, -1, 0), (1, 1, 0, 2, 0), (0, 0, 0, -1, 2), (1, 0, 0, -1, 0)]],
}


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('variant', [0, 1])
@pytest.mark.parametrize('geom', [(6, 37, 61), (4, 160, 192)])
def test_route_labels_vs_numpy(dev, geom, variant, aligned):
    """Exact equality with the numpy restatement; the label rows, every destination, overlay and feed lie between guard bytes,
    which must survive.  aligned: the rows start at a multiple of 4 and so does every operand, so at (4, 160, 192) -- the rows are
    30720 bytes -- EVERY live row takes the 32-bit loads and stores (the path of every production call), with feed, overlay,
    feed + overlay, delivery and the byte-reversed twin store; at (6, 37, 61), 2257 bytes a row, rows 0 and 4 do and the others
    start at 1, 2, 3 mod 4.  Not aligned: rows from byte 61 and operands at 64 + 3 r + k, the byte path and the mixed cases."""
    from rmem_ocu_amd import ops
    rows, Ho, Wo = geom
    n = Ho * Wo
    rng = np.random.default_rng(rows * 1000 + variant)
    spec = TABLES[rows][variant]
    front = 64 if aligned else 61
    buf = torch.full((front + rows * n + 4096,), CANARY, dtype=torch.uint8)
    rows0 = rng.integers(0, 11, (rows, Ho, Wo)).astype(np.uint8)
    buf[front:front + rows * n] = torch.from_numpy(rows0).reshape(-1)
    buf = buf.to(dev)
    rows_u8 = buf[front:front + rows * n].view(rows, Ho, Wo)

    def operand(r, which, sparse=False):
        """A map of its own between guards, at offset 64 + 4 (3 r + which) (aligned) or 64 + 3 r + which."""
        off = 64 + (4 if aligned else 1) * (3 * r + which)
        a = rng.integers(0, 11, (Ho, Wo)).astype(np.uint8)
        if sparse:
            a[rng.random((Ho, Wo)) < 0.7] = 0
        t = torch.full((off + n + 256,), CANARY, dtype=torch.uint8)
        t[off:off + n] = torch.from_numpy(a).reshape(-1)
        t = t.to(dev)
        return a, t, t[off:off + n].view(Ho, Wo)

    table, routes, guards = [], [], []
    for r, (delivers, has_ov, has_fd, twin, mode) in enumerate(spec):
        dst = operand(r, 0) if delivers else None
        ov = operand(r, 1, sparse=True) if has_ov else None
        fd = operand(r, 2) if has_fd else None
        table.append((delivers, ov[0] if ov else None, fd[0] if fd else None, twin, mode))
        routes.append((dst[2] if dst else None, ov[2] if ov else None, fd[2] if fd else None, twin, mode))
        guards.append((dst, ov, fd))
    lr = ops.LabelRoutes(rows_u8, dev)
    s = torch.cuda.current_stream().cuda_stream
    lr.upload(routes, s)
    lr.op(s)
    torch.cuda.synchronize()
    want_rows, want_out = _route_ref(rows0, table)
    got = buf.cpu().numpy()
    assert (got[:front] == CANARY).all() and (got[front + rows * n:] == CANARY).all(), 'guard bytes around the label rows'
    assert np.array_equal(got[front:front + rows * n].reshape(rows, Ho, Wo), want_rows)
    step = 4 if aligned else 1
    if aligned:
        assert rows_u8.data_ptr() % 4 == 0 and all(t[2].data_ptr() % 4 == 0 for g in guards for t in g if t is not None)
    for r, (dst, ov, fd) in enumerate(guards):
        off = 64 + step * 3 * r
        if dst is not None:
            d = dst[1].cpu().numpy()
            assert (d[:off] == CANARY).all() and (d[off + n:] == CANARY).all(), f'row {r}: guard bytes around the destination'
            assert np.array_equal(d[off:off + n].reshape(Ho, Wo), want_out[r]), f'row {r}: delivered map'
        for k, src in ((1, ov), (2, fd)):                         # inputs are read only
            if src is not None:
                t, o = src[1].cpu().numpy(), off + step * k
                assert np.array_equal(t[o:o + n].reshape(Ho, Wo), src[0]) and (t[:o] == CANARY).all() and (t[o + n:] == CANARY).all()


def test_route_labels_refuses_a_bad_table_on_the_host(dev):
    from rmem_ocu_amd import ops
    from rmem_ocu_amd._lib import RmemError
    rows_u8 = torch.full((3, 8, 12), 7, dtype=torch.uint8, device=dev)
    lr = ops.LabelRoutes(rows_u8, dev)
    s = torch.cuda.current_stream().cuda_stream
    idle = (None, None, None, -1, 1)
    with pytest.raises(RmemError, match='twin'):                 # the twin's own entry must be skipped
        lr.upload([(None, None, None, 1, 0), idle, idle], s)
    with pytest.raises(RmemError, match='twin'):
        lr.upload([(None, None, None, 3, 0), idle, idle], s)
    with pytest.raises(RmemError, match='uint8 map'):
        lr.upload([(torch.zeros(8, 11, dtype=torch.uint8, device=dev), None, None, -1, 0), idle, idle], s)
    with pytest.raises(RmemError, match='entries'):
        lr.upload([idle], s)
    torch.cuda.synchronize()
    assert (rows_u8 == 7).all(), 'a refused table launched'


# ---------------------------------------------------------------------------------------------------------------- engine + slot
@functools.lru_cache(maxsize=None)
def _model(name='r50_aotl'):
    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.weights import synth_state_dict
    cfg = get_config('pre_vost', 'test', name)
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 7
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0, model='deaot' if name == 'r50_deaotl' else 'aot'))
    return model


@functools.lru_cache(maxsize=None)
def _clip(n, seed=None):
    from rmem_ocu_amd.synth import make_clip
    return make_clip(300 + n if seed is None else seed, n, NET[0], NET[1], OBJS)


def _new_object():
    new = torch.zeros(OUT, dtype=torch.uint8)
    new[OUT[0] // 2:OUT[0] // 2 + OUT[0] // 4, OUT[1] // 8:OUT[1] // 8 + OUT[1] // 5] = OBJS + 1
    return new


@functools.lru_cache(maxsize=None)
def _reference(n, gap, name='r50_aotl', new_at=None):
    """The per-clip engine's (labels [n - 1, Ho, Wo], long_memories_indexes per frame) of clip n: computed once, shared, read only."""
    from test_hip_engine import _per_clip_reference
    f, m = _clip(n)
    new = (new_at, _new_object()) if new_at is not None else None
    return _per_clip_reference(1, 7, gap, f, m, OBJS, OUT, new_object=new, model_name=name)


def _ragged_run(dev, lengths, rows, lookahead, gaps=None, name='r50_aotl', new_objects=None, sync=True, frames=None, engine=None,
                check_idle=False):
    """The clips of ``lengths`` through a RaggedGroupSlot of ``rows`` rows -> ({clip: FinishedClip}, {clip: trace per frame}, slot,
    engine, [(step, clip) of every row start]).  sync: wait for the engine after every step and record every live row's index list."""
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    ge = engine or GroupEngine(_model(name), rows, 0, lookahead=lookahead)
    slot = RaggedGroupSlot(ge, OUT, dev)
    for j, n in enumerate(lengths):
        f, m = _clip(n)
        src = frames[j] if frames is not None else f.to(dev)
        slot.submit(j, src, m.to(dev), new_objects=(new_objects or {}).get(j), gap=2 if gaps is None else gaps[j])
    fins, traces, starts, step = {}, {j: [] for j in range(len(lengths))}, [], 0
    while not slot.done:
        queued = bool(slot._queue)
        before = {id(r.clip) for r in slot._rows if r.live}
        for fin in slot.step():
            assert fin.clip_id not in fins
            fins[fin.clip_id] = fin
            traces[fin.clip_id].append(list(fin.long_memories_indexes))
        step += 1
        starts += [(step, r.clip.id) for r in slot._rows if r.live and id(r.clip) not in before]
        if sync:
            ge.synchronize()
            for p, r in enumerate(slot._rows):
                if r.live:
                    traces[r.clip.id].append(list(ge.long_memories_indexes(p)))
        if check_idle and queued:                                   # test 9: a row waits for its next clip at most one batch
            assert slot.row_steps_idle <= slot.refills * (lookahead - 1), (step, slot.row_steps_idle, slot.refills)
    ge.synchronize()
    assert sorted(fins) == list(range(len(lengths)))
    return fins, traces, slot, ge, starts


def _check(fins, traces, lengths, gaps=None, name='r50_aotl', new_at=None, what=''):
    """Every clip of the list against its per-clip reference: labels >= 0.995, traces equal at every frame."""
    for j, n in enumerate(lengths):
        ref_labels, ref_trace = _reference(n, 2 if gaps is None else gaps[j], name, (new_at or {}).get(j))
        got = fins[j].labels.cpu().numpy()
        assert got.shape == (n, *OUT) and not got[0].any()
        agree = (got[1:] == ref_labels).mean()
        print(f'{what} clip {j} ({n} frames): label agreement {agree:.5f}, final indexes {traces[j][-1]}, drops {fins[j].drop_trace}')
        assert agree >= 0.995, (what, j, agree)
        assert traces[j] == ref_trace, (what, j, traces[j][-1], ref_trace[-1])


_RUNS = {}


def _parity_run(dev, lookahead):
    if lookahead not in _RUNS:
        _RUNS[lookahead] = _ragged_run(dev, LENGTHS, 2, lookahead, check_idle=True)
    return _RUNS[lookahead]


@pytest.mark.parametrize('lookahead', [1, 2])
def test_ragged_group_matches_per_clip_engines(dev, lookahead):
    """Two rows, five clips of (9, 30, 14, 22, 12) frames: the 30-frame clip is evicting (from frame 16 on) while its neighbour row
    is refilled; also the idle-step bound (with look-ahead 1 no row ever idles while clips are queued)."""
    fins, traces, slot, ge, starts = _parity_run(dev, lookahead)
    _check(fins, traces, LENGTHS, what=f'look-ahead {lookahead}')
    assert fins[1].drop_trace and any(16 < step <= 29 for step, clip in starts if clip >= 2), starts
    assert slot.refills == 3 and slot.row_steps_live == sum(LENGTHS) - len(LENGTHS)


def test_ragged_group_clip_shorter_than_a_batch(dev):
    """Look-ahead 4 with a 3-frame clip in the list: it starts and ends inside one look-ahead batch."""
    lengths = (9, 30, 3, 14)
    fins, traces, slot, ge, _ = _ragged_run(dev, lengths, 2, 4, check_idle=True)
    _check(fins, traces, lengths, what='look-ahead 4')
    assert slot.refills == 2


def test_ragged_group_per_clip_gaps(dev):
    """Gaps 2 and 3 side by side in one group, each clip against the reference run with its gap."""
    lengths, gaps = (14, 22, 12, 9), (2, 3, 3, 2)
    fins, traces, slot, ge, _ = _ragged_run(dev, lengths, 2, 2, gaps=gaps)
    _check(fins, traces, lengths, gaps=gaps, what='gaps')
    assert traces[1][-1] == [0] + list(range(3, 22, 3)) and traces[0][-1] == [0] + list(range(2, 14, 2))


def test_ragged_group_new_object_while_the_other_row_refills(dev):
    """A new object's mask arrives at frame 7 of the clip in row 0 (mid-clip reference frame: bank back to one entry, index list
    keeps growing) in the look-ahead batch at whose boundary row 1 takes its next clip."""
    lengths = (22, 7, 12)
    new = _new_object().to(dev)
    fins, traces, slot, ge, starts = _ragged_run(dev, lengths, 2, 2, new_objects={0: {7: new}})
    assert (7, 2) in starts, starts                                  # clip 2 moves in at the step that propagates frame 7 of clip 0
    _check(fins, traces, lengths, new_at={0: 7}, what='new object')
    assert (fins[0].labels[7][new > 0] == OBJS + 1).all() and (new > 0).sum() > 0        # the overlay is in the delivered map


def test_ragged_flip_group_matches_sequence_evaluator(dev):
    """GroupEngine(flip_tta=True) of four rows = two clips and their mirrored twins, three clips of (10, 17, 13) frames against
    SequenceEvaluator(flip=True) clip by clip, as test_hip_flip_group.py does: labels, and the traces of the plain and the
    flipped engine for the clip's row and its twin's."""
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from test_hip_flip_group import _evaluator_runs, _first_masks
    lengths = (10, 17, 13)
    model = _model()
    frames, firsts, nets = [], [], []
    for n in lengths:
        f, m = _clip(n)
        first, net = _first_masks(m, OUT, NET, dev)
        frames.append(f.to(dev)); firsts.append(first); nets.append(net)
    refs = _evaluator_runs(model, list(zip(frames, firsts)), OUT, dev)
    ge = GroupEngine(model, 4, 0, lookahead=2, flip_tta=True)
    slot = RaggedGroupSlot(ge, OUT, dev)
    for j in range(3):
        slot.submit(j, frames[j], nets[j])                          # the evaluator's gap: max(round(n / 30), 5)
    fins = {}
    while not slot.done:
        for fin in slot.step():
            fins[fin.clip_id] = fin
        ge.synchronize()
        P = slot.clips
        live = [p for p, r in enumerate(slot._rows) if r.live]
        assert all(torch.equal(slot.cur_label[P + p], slot.cur_label[p].flip(-1)) for p in live), 'twin rows are not the mirror'
    assert sorted(fins) == [0, 1, 2]
    for j, (ref_labels, ref_traces) in enumerate(refs):
        got = fins[j].labels.cpu().numpy()
        agree = (got[1:] == ref_labels).mean()
        print(f'flip clip {j}: label agreement {agree:.5f}, indexes {fins[j].long_memories_indexes} / {fins[j].twin_traces[0]}')
        assert agree >= 0.995
        assert (fins[j].long_memories_indexes, fins[j].drop_trace) == ref_traces[0], j
        assert tuple(fins[j].twin_traces) == ref_traces[1], j


def test_ragged_group_deaot(dev):
    """R50-DeAOTL (group_runtime_deaot; the policy state moves on every update): two rows, three clips; the 24-frame clip moves
    into a used row and evicts there."""
    lengths = (9, 12, 24)
    fins, traces, slot, ge, _ = _ragged_run(dev, lengths, 2, 2, name='r50_deaotl')
    _check(fins, traces, lengths, name='r50_deaotl', what='deaot')
    assert slot.refills == 1 and fins[2].drop_trace


def test_ragged_group_from_pinned_uint8_frames(dev):
    """Clips fed from uint8 frames in pinned host memory give exactly the labels of the same clips fed with the ingested fp32 frames
    from device memory (the bar of test_group_slot_from_pinned_uint8_frames), with and without look-ahead."""
    from rmem_ocu_amd import ops
    lengths = (9, 12, 3, 14)
    u8s, ings = [], []
    for n in lengths:
        f, _ = _clip(n)
        vid = F.interpolate(f, size=OUT, mode='bilinear', align_corners=False)
        u8 = (vid * 40.0 + 128.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()
        u8d = u8.to(dev)
        ing = torch.empty(n, 3, *NET, dtype=torch.float32, device=dev)
        ops.run([ops.ingest_rgb8(u8d[i], Hs=OUT[0], Ws=OUT[1], Hd=NET[0], Wd=NET[1], out_chw=ing[i]) for i in range(n)])
        u8s.append(u8); ings.append(ing)
    torch.cuda.synchronize()
    for la in (2, 1):
        a = _ragged_run(dev, lengths, 2, la, frames=ings, sync=False)[0]
        b = _ragged_run(dev, lengths, 2, la, frames=u8s, sync=False)[0]
        for j in range(len(lengths)):
            assert torch.equal(a[j].labels[1:], b[j].labels[1:]), (la, j)
            assert a[j].labels[1:].any()


def test_ragged_flip_group_from_pinned_uint8_frames(dev):
    """A flip group of four rows (two clips and their twins) fed from pinned uint8 frames, clips of (9, 12, 3) frames, with and
    without look-ahead: exactly the labels of the same run fed with the ingested fp32 frames (the bar of
    test_ragged_group_from_pinned_uint8_frames), and after every step the twin rows of cur_label are the mirror of the clips'."""
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    lengths = (9, 12, 3)
    u8s, ings, masks = [], [], []
    for n in lengths:
        f, m = _clip(n)
        vid = F.interpolate(f, size=OUT, mode='bilinear', align_corners=False)
        u8 = (vid * 40.0 + 128.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()
        u8d = u8.to(dev)
        ing = torch.empty(n, 3, *NET, dtype=torch.float32, device=dev)
        ops.run([ops.ingest_rgb8(u8d[i], Hs=OUT[0], Ws=OUT[1], Hd=NET[0], Wd=NET[1], out_chw=ing[i]) for i in range(n)])
        u8s.append(u8); ings.append(ing); masks.append(m.to(dev))
    torch.cuda.synchronize()

    def run(la, frames):
        ge = GroupEngine(_model(), 4, 0, lookahead=la, flip_tta=True)
        slot = RaggedGroupSlot(ge, OUT, dev)
        for j in range(len(lengths)):
            slot.submit(j, frames[j], masks[j], gap=2)
        fins, P = {}, slot.clips
        while not slot.done:
            for fin in slot.step():
                fins[fin.clip_id] = fin
            ge.synchronize()
            live = [p for p, r in enumerate(slot._rows) if r.live]
            assert all(torch.equal(slot.cur_label[P + p], slot.cur_label[p].flip(-1)) for p in live), 'twin rows are not the mirror'
        assert sorted(fins) == list(range(len(lengths)))
        return fins

    for la in (2, 1):
        a, b = run(la, ings), run(la, u8s)
        for j in range(len(lengths)):
            assert torch.equal(a[j].labels[1:], b[j].labels[1:]), (la, j)
            assert a[j].labels[1:].any()


def test_ragged_group_table_uploads_never_race_the_gpu(dev):
    """Key table, append table, encoder frame table and the label-route table are re-sent through pinned rings every step while
    earlier steps are still queued.  A run that never synchronises delivers exactly the labels of a run that synchronises after
    every step (test_group_engine_table_uploads_never_race_the_gpu); gap 1, so every table changes every frame."""
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    gaps = (1,) * len(LENGTHS)
    synced = _ragged_run(dev, LENGTHS, 2, 2, gaps=gaps, sync=True)[0]
    ge = GroupEngine(_model(), 2, 0, lookahead=2)
    _ragged_run(dev, LENGTHS, 2, 2, gaps=gaps, sync=False, engine=ge)          # builds every graph, so that the racing run only replays
    racing = _ragged_run(dev, LENGTHS, 2, 2, gaps=gaps, sync=False, engine=ge)[0]
    for j in range(len(LENGTHS)):
        assert racing[j].long_memories_indexes == synced[j].long_memories_indexes and racing[j].drop_trace == synced[j].drop_trace
        assert torch.equal(racing[j].labels, synced[j].labels), f'clip {j}: asynchronous table uploads changed the masks'


def test_ragged_group_idle_steps_are_bounded(dev):
    """While clips are queued a row idles at most look-ahead - 1 steps per refill (asserted at every step of the parity runs); with
    look-ahead 1 never.  Occupancy follows from the counters."""
    for la in (1, 2):
        slot = _parity_run(dev, la)[2]
        assert slot.refills == 3
        assert (slot.row_steps_live + slot.row_steps_idle) % 2 == 0          # two rows per step, live or idle
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    ge = GroupEngine(_model(), 2, 0, lookahead=1)
    slot = RaggedGroupSlot(ge, OUT, dev)
    for j, n in enumerate((9, 3, 14, 3)):
        f, m = _clip(n)
        slot.submit(j, f.to(dev), m.to(dev), gap=2)
    while not slot.done:
        queued = bool(slot._queue)
        slot.step()
        if queued:
            assert slot.row_steps_idle == 0
    ge.synchronize()
    assert slot.refills == 2 and slot.row_steps_live == 8 + 2 + 13 + 2


def test_ragged_group_feed(dev):
    """step(feed=...) as GroupSlot.step: the delivered labels stay the prediction, the memory continues from the given labels.
    Fed the per-clip reference's own labels, every frame is an independent comparison against that reference (labels >= 0.995,
    traces equal), for a clip that moves into a used row too; fed labels that are NOT the prediction (all zero) for one clip,
    that clip's later predictions change while its neighbour's do not."""
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    lengths = (9, 14, 12)
    refs = [torch.from_numpy(_reference(n, 2)[0]).to(dev) for n in lengths]

    def run(feed_of):
        ge = GroupEngine(_model(), 2, 0, lookahead=2)
        slot = RaggedGroupSlot(ge, OUT, dev)
        for j, n in enumerate(lengths):
            f, m = _clip(n)
            slot.submit(j, f.to(dev), m.to(dev), gap=2)
        fins, traces = {}, {j: [] for j in range(len(lengths))}
        while not slot.done:
            # the frame a row propagates in this step: a live row's next one, frame 1 for a clip that starts in this step
            nxt = {r.clip.id: r.i for r in slot._rows if r.live and r.i < r.clip.n}
            feed = {j: feed_of(j, nxt.get(j, 1)) for j in range(len(lengths))}
            for fin in slot.step(feed={j: t for j, t in feed.items() if t is not None}):
                fins[fin.clip_id] = fin
                traces[fin.clip_id].append(list(fin.long_memories_indexes))
            ge.synchronize()
            for p, r in enumerate(slot._rows):
                if r.live:
                    traces[r.clip.id].append(list(ge.long_memories_indexes(p)))
        return fins, traces

    fins, traces = run(lambda j, i: refs[j][i - 1].contiguous())
    _check(fins, traces, lengths, what='fed the reference labels')
    zero = torch.zeros(OUT, dtype=torch.uint8, device=dev)
    free = _ragged_run(dev, lengths, 2, 2)[0]
    other, _ = run(lambda j, i: zero if j == 1 else None)
    assert torch.equal(other[0].labels, free[0].labels), 'feeding clip 1 changed clip 0'
    assert torch.equal(other[1].labels[1], free[1].labels[1]) and not torch.equal(other[1].labels[2:], free[1].labels[2:])


def test_run_clips(dev):
    """evaluator.run_clips yields every clip id once; for two clips its stacks are those of a RaggedGroupSlot driven by hand with
    the same settings (default gaps), and that run meets the per-clip bar at gap 5."""
    from rmem_ocu_amd.evaluator import run_clips
    clips = []
    for j, n in enumerate(LENGTHS):
        f, m = _clip(n)
        clips.append((f'clip{j}', f.to(dev), m.to(dev), None))
    got = {}
    for cid, lab in run_clips(_model(), iter(clips), rows=2, lookahead=2, out_hw=OUT):
        assert cid not in got
        got[cid] = lab
    torch.cuda.synchronize()
    assert sorted(got) == [f'clip{j}' for j in range(len(LENGTHS))]
    for j in range(len(LENGTHS)):
        assert got[f'clip{j}'].shape == (LENGTHS[j], *OUT)
    gaps = (None, None)                                           # the evaluator's gap, max(round(n / 30), 5) = 5
    fins, traces, _, _, _ = _ragged_run(dev, LENGTHS[:2], 2, 2, gaps=gaps)
    _check(fins, traces, LENGTHS[:2], gaps=(5, 5), what='default gaps')
    two = dict(run_clips(_model(), clips[:2], rows=2, lookahead=2, out_hw=OUT))
    torch.cuda.synchronize()
    for j in range(2):
        assert torch.equal(two[f'clip{j}'], fins[j].labels), j
        assert torch.equal(got[f'clip{j}'], fins[j].labels), j
