"""Host side of ragged clip groups (no GPU): the per-row bank schedule against one-clip schedules run alone, idle rows, and the
refusals of rmem_route_labels and clip_runner.RaggedGroupSlot."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from test_host_logic import _StandInBank, _schedule_traces, _scores


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _ragged_schedule(rows, N, every):
    """A ``rows``-row BankSchedule driven the way RaggedGroupSlot drives it: (rt, engine stand-in, schedule, log).  log['scored'] and
    log['T'] record what the score readback was asked for."""
    from rmem_ocu_amd.bank_schedule import BankSchedule, bank_slots
    eng = NS(frame_step=0, long_term_mem_gap=9999, policy_every_update=every, stream=NS(cuda_stream=0),
             cfg=NS(FORMER_MEM_LEN=1, LATTER_MEM_LEN=N - 1))
    rt = _StandInBank(rows, bank_slots(N))
    log = {'scored': [], 'stream': [None] * rows}

    def score(rt, stream, scored, T, keep):
        log['scored'].append(list(scored))
        for c in scored:
            Tc = len(rt.slots[c]) - 1
            assert Tc <= T
            mass, fg = _scores(log['stream'][c], sch.step_of(c), Tc)      # the clip's own stream at the clip's own frame index
            rt.scores_host[c, :Tc] = (mass * fg[:, None]).sum(0)
        return NS(synchronize=lambda: None)

    sch = BankSchedule(eng, rows, score=score)
    return rt, eng, sch, log


@pytest.mark.parametrize('N', [3, 8])
@pytest.mark.parametrize('every', [False, True])
def test_ragged_schedule_equals_solo_schedules(N, every):
    """Three rows, >= 120 steps, clips of 9..45 frames with gaps from {1, 2, 3, 5} moving into rows at different steps (a row idles
    0..2 steps before its next clip): every clip's per-frame (long_memories_indexes, drop_trace) is that of a one-clip schedule run
    alone with that gap, counted from the clip's own frame 0; at least one clip evicts after it was moved into a used row."""
    rows = 3
    rng = np.random.default_rng(11 + N)
    clips = [(sid, int(rng.integers(9, 46)), int(rng.choice([1, 2, 3, 5]))) for sid in range(40)]
    clips[3] = (3, 45, 1)                      # refills that certainly evict, whatever the draw
    clips[5] = (5, 44, 2)
    assert {g for _, _, g in clips} == {1, 2, 3, 5} and min(n for _, n, _ in clips) >= 9 and max(n for _, n, _ in clips) <= 45
    rt, eng, sch, log = _ragged_schedule(rows, N, every)
    queue = list(clips)
    state = [None] * rows                      # per row: [stream id, n, gap, next frame, trace, is refill] or None
    wait = [0] * rows
    used = [False] * rows
    finished = {}
    steps = 0

    def fill():
        new = [r for r in range(rows) if state[r] is None and wait[r] == 0 and queue]
        if not new:
            return
        picked = [queue.pop(0) for _ in new]
        for r, (sid, n, gap) in zip(new, picked):
            state[r] = [sid, n, gap, 1, [], used[r]]
            log['stream'][r] = sid
            used[r] = True
        first = sch.start_clips(rt, new, [g for _, _, g in picked])
        assert all(first[r] >= 0 for r in new) and all(len(rt.slots[r]) == 1 for r in new)

    fill()
    while any(s is not None for s in state) or queue:
        live = [r for r in range(rows) if state[r] is not None]
        if live:
            eng.frame_step += 1
            sch.advance()
            T, _ = sch.begin_propagation(rt)
            assert T == max(len(rt.slots[r]) for r in live)                     # idle rows never lengthen T
            slots = sch.take_append_slots(rt)
            assert all(slots[r] == -1 for r in range(rows) if r not in live)
            before = len(log['scored'])
            sch.commit_update(rt, slots, keep=10)
            assert all(set(s) <= set(live) for s in log['scored'][before:])
            ended = []
            for r in live:
                st = state[r]
                assert sch.step_of(r) == st[3]
                st[4].append((list(sch.long_memories_indexes(r)), list(sch.drop_trace[r])))
                st[3] += 1
                if st[3] >= st[1]:
                    ended.append(r)
            for r, tr in zip(ended, sch.finish_clips(rt, ended)):
                st = state[r]
                assert tr == st[4][-1] and len(rt.slots[r]) == 1
                finished[st[0]] = st
                state[r] = None
                wait[r] = int(rng.integers(0, 3))
            steps += 1
        fill()
        wait = [max(w - 1, 0) if state[r] is None else 0 for r, w in enumerate(wait)]
    assert steps >= 120 and len(finished) == len(clips)
    evicted_after_refill = 0
    for sid, n, gap in clips:
        st = finished[sid]
        solo = _schedule_traces([sid], N, gap, n, {}, every)
        assert st[4] == [fr[0] for fr in solo], (N, every, sid, n, gap)
        evicted_after_refill += bool(st[5] and st[4][-1][1])
    assert evicted_after_refill >= 1


def test_new_clip_in_a_row_evicts_where_a_mid_clip_reference_raises():
    """start_reference keeps the row's index list growing (the reference's quirk), so the restarted bank's first eviction raises
    (DESIGN.md section 2); a NEW clip in the row starts over and evicts like a clip on a fresh schedule."""
    for new_clip in (False, True):
        rt, eng, sch, log = _ragged_schedule(1, 2, False)
        log['stream'][0] = 0
        sch.start_clips(rt, [0], [1])

        def frames(k):
            for _ in range(k):
                eng.frame_step += 1
                sch.advance()
                sch.begin_propagation(rt)
                sch.commit_update(rt, sch.take_append_slots(rt), keep=10)
                sch.resolve()

        frames(6)
        assert len(sch.drop_trace[0]) == 5
        if new_clip:
            assert sch.finish_clips(rt, [0])[0][1] == sch.drop_trace[0]
            log['stream'][0] = 1
            sch.start_clips(rt, [0], [1])
            frames(6)
            assert sch.long_memories_indexes(0)[0] == 0 and len(sch.drop_trace[0]) == 5
        else:
            sch.start_reference(rt, [0], append_table=False)
            with pytest.raises(RuntimeError):
                frames(6)


def test_idle_rows_never_append_are_never_scored_and_never_lengthen_T():
    rt, eng, sch, log = _ragged_schedule(3, 4, True)
    for r in range(3):
        log['stream'][r] = r
    sch.start_clips(rt, [0, 1, 2], [1, 1, 2])

    def frame():
        eng.frame_step += 1
        sch.advance()
        T, _ = sch.begin_propagation(rt)
        lens = [len(sl) for sl in rt.slots]                     # the banks the launches of this frame read
        slots = sch.take_append_slots(rt)
        sch.commit_update(rt, slots, keep=10)
        return T, slots, lens

    for _ in range(6):
        frame()
    idx, drops = sch.finish_clips(rt, [1])[0]
    assert idx[0] == 0 and len(idx) == 4 and drops
    seen = len(log['scored'])
    kept = list(rt.slots[1])
    for _ in range(40):                                         # far beyond the runtime's slots: an appending row would raise
        T, slots, lens = frame()
        assert slots[1] == -1 and rt.slots[1] == kept and len(kept) == 1
        assert T == max(lens[0], lens[2]) and lens[1] == 1
        assert sch.step_of(1) == 6                              # an idle row's frame counter stands still
    assert all(1 not in s for s in log['scored'][seen:]) and len(log['scored']) > seen
    sch.finish_clips(rt, [0, 2])                                # all rows idle: T is the shortest bank there is
    T, slots, _ = frame()
    assert T == 1 and slots == [-1, -1, -1]


def test_route_labels_refuses_bad_arguments_without_a_gpu(lib):
    """Refused on the host before anything is launched (the pointers are never dereferenced)."""
    from rmem_ocu_amd import _lib, ops
    from rmem_ocu_amd._lib import RmemError
    assert 'rmem_route_labels' in _lib.SIGNATURES and 'rmem_route_labels' not in _lib.F16_TWINS

    def call(rows_u8, rows, Ho, Wo, routes):
        return lib.rmem_route_labels(rows_u8, rows, Ho, Wo, routes, None)
    assert call(4096, 0, 8, 8, 4096) != 0 and b'rows' in lib.rmem_last_error_string()
    assert call(4096, -3, 8, 8, 4096) != 0 and b'rows' in lib.rmem_last_error_string()
    assert call(None, 2, 8, 8, 4096) != 0 and b'null' in lib.rmem_last_error_string()
    assert call(4096, 2, 8, 8, None) != 0 and b'null' in lib.rmem_last_error_string()
    assert call(4096, 2, 0, 8, 4096) != 0 and b'positive' in lib.rmem_last_error_string()
    assert call(4096, 2, 8, -1, 4096) != 0 and b'positive' in lib.rmem_last_error_string()
    import ctypes
    assert ctypes.sizeof(_lib.LabelRoute) == 32                 # three pointers, twin, mode: what ops.LabelRoutes packs per row
    rows_u8, table = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RmemError, match='positive'):
        ops.route_labels(rows_u8, table, rows=0, Ho=8, Wo=8)
    with pytest.raises(RmemError, match='device tensors'):      # and, as every op, no CPU fallback
        ops.route_labels(rows_u8, table, rows=2, Ho=8, Wo=8)


def test_ragged_group_slot_refusals():
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    from rmem_ocu_amd.jpeg import JpegClip
    slot = RaggedGroupSlot(NS(B=2, lookahead=2, flip_tta=False), (16, 18), torch.device('cpu'))
    mask = torch.zeros(1, 1, 17, 19)
    with pytest.raises(ValueError, match='JpegClip'):
        slot.submit('j', object.__new__(JpegClip), mask)
    slot.submit('a', torch.zeros(3, 3, 17, 19), mask)
    with pytest.raises(ValueError, match='network size'):
        slot.submit('b', torch.zeros(3, 3, 33, 19), torch.zeros(1, 1, 33, 19))
    with pytest.raises(ValueError, match='size of the first mask'):
        slot.submit('c', torch.zeros(3, 3, 33, 19), mask)
    slot.submit('d', torch.zeros(5, 3, 17, 19), mask, gap=3)
    assert [c.id for c in slot._queue] == ['a', 'd'] and not slot.done
    assert [c.gap for c in slot._queue] == [5, 3] and slot._queue[1].labels.shape == (5, 16, 18)
