"""Host side of frame_feed.FrameFeed (no GPU): the row table of a look-ahead batch of fp32 sources, the gap rule, and what the
feed refuses or leaves alone before any launch."""
from types import SimpleNamespace as NS

import pytest
import torch


def _clip(n):
    return NS(shape=(n, 3, 17, 19))                     # lookahead_rows reads the frame count only


@pytest.mark.parametrize('flip', [False, True])
def test_lookahead_rows_equal_length_plan_is_the_group_slot_layout(flip):
    """P = 2 clips of 5 frames, look-ahead 3, first index 3 (m = 2): GroupSlot's table, written out -- row k * B + c is frame
    min(3 + k, 4) of clip c, the twin's row k * B + P + c is twin staging [c, min(k, m - 1)]."""
    from rmem_ocu_amd.frame_feed import lookahead_rows
    P, la = 2, 3
    B = 2 * P if flip else P
    plan = {c: (_clip(5), 3, None) for c in range(P)}
    want = []
    for k, (frame, staged) in enumerate([(3, 0), (4, 1), (4, 1)]):
        want += [('frame', 0, frame), ('frame', 1, frame)]
        if flip:
            want += [('twin', 0, staged), ('twin', 1, staged)]
    got = lookahead_rows(plan, B, P, la, flip)
    assert len(got) == la * B and got == want


def test_lookahead_rows_ragged_plan():
    """Three rows with flip: row 0 runs on (frames 4, 5, 6 of 9), row 1 has no plan, row 2's clip ends after one frame of the batch
    (frame 6 of 7: repeated, and its twin staging row 0 repeated)."""
    from rmem_ocu_amd.frame_feed import lookahead_rows
    P, la, B = 3, 3, 6
    plan = {0: (_clip(9), 4, None), 2: (_clip(7), 6, object())}
    got = lookahead_rows(plan, B, P, la, True)
    assert len(got) == la * B
    for k in range(la):
        row = got[k * B:(k + 1) * B]
        assert row[0] == ('frame', 0, 4 + k) and row[P + 0] == ('twin', 0, k)
        assert row[1] == ('idle',) and row[P + 1] == ('idle',)
        assert row[2] == ('frame', 2, 6) and row[P + 2] == ('twin', 2, 0)
    assert all(e == ('idle',) or e[1] in plan for e in got)
    # without flip the same plan fills B = P rows per frame index and names no twin
    plain = lookahead_rows(plan, P, P, la, False)
    assert plain == [e for k in range(la) for e in got[k * B:k * B + P]]


def test_clip_gap():
    """max(round(n / 30), 5); Python rounds half to even: round(5.5) = 6, round(6.5) = 6."""
    from rmem_ocu_amd.clip_runner import clip_gap
    assert [clip_gap(n) for n in (1, 149, 150, 165, 195)] == [5, 5, 5, 6, 6]


def test_feed_allocates_nothing_at_construction_and_refuses_unpinned_frames():
    from rmem_ocu_amd.clip_runner import GroupSlot, RaggedGroupSlot
    from rmem_ocu_amd.frame_feed import FrameFeed
    feed = FrameFeed('cpu', B=4, P=2, lookahead=2, flip=True)
    assert feed._bufs == {} and feed._zeroed_rt is None
    stage = feed.stage(2, 8, 10)
    assert stage.shape == (2, 8, 10, 3) and stage.dtype == torch.uint8 and feed.stage(2, 8, 10) is stage
    assert feed.stage(2, 6, 10) is not stage                            # a new size: allocated again
    first = feed.rows('first', (4, 3, 17, 19), zero=True)
    assert first.dtype == torch.float32 and not first.any() and feed.rows('first', (4, 3, 17, 19)) is first
    u8 = torch.zeros(3, 8, 10, 3, dtype=torch.uint8)
    feed.check_pinned(u8)                                               # a feed on the CPU stages nothing: no pinning asked for
    with pytest.raises(ValueError, match='uint8 host frames must be in pinned memory'):
        FrameFeed('cuda').check_pinned(u8)
    # the slots own a feed and build it without touching a device
    eng = NS(B=4, lookahead=2, flip_tta=True)
    for slot in (GroupSlot(eng, (16, 18), 'cpu'), RaggedGroupSlot(eng, (16, 18), torch.device('cpu'))):
        assert slot.feed._bufs == {} and (slot.feed.B, slot.feed.P, slot.feed.lookahead, slot.feed.flip) == (4, 2, 2, True)
    # ... and the ragged slot refuses an unpinned clip at submit, through its feed
    slot = RaggedGroupSlot(NS(B=2, lookahead=2, flip_tta=False), (16, 18), torch.device('cpu'))
    slot.feed = FrameFeed('cuda', 2, 2, 2)
    with pytest.raises(ValueError, match='uint8 host frames must be in pinned memory'):
        slot.submit('u', u8, torch.zeros(1, 1, 17, 19))
    assert not slot._queue
