"""Host-side schedule of the restricted memory bank, once, for the per-clip engines (clips = 1) and GroupEngine (clips = B).

What the reference keeps in Python (networks/engines/aot_engine.py:318-369, networks/layers/transformer.py:324-443): the
"append every ``gap`` frames" rule, which bank slot a new entry takes, when a bank overflows, the eviction policy
(``MemoryPolicy``), ``long_memories_indexes`` and the reset of a bank to one entry by a reference frame.  The decisions are
host arithmetic on the runtime's ``slots`` / ``free`` lists; the device work they trigger is three actions -- the chunk (key)
table upload and the append table upload of the runtime, and the score reduction + readback (``device_scores``) -- so a
stand-in for those drives the whole schedule without a GPU (tests/test_host_logic.py).

The eviction decision is deferred: ``commit_update`` only issues the score readback, ``resolve`` takes the decision right
before the bank is used again, so the host never waits in the update.  Between the two a restricted bank holds N + 1 entries
(``bank_slots``).

RAGGED groups (clip_runner.RaggedGroupSlot): the rows of a group may run clips of different lengths, each at its own frame index
with its own gap.  A row then has a frame counter and a gap of its own (``row_step`` / ``row_gap``, set by ``start_clips``, moved
by ``advance``); a row without them reads the owner's shared ``frame_step`` / ``long_term_mem_gap``, so an engine that never
starts a clip per row behaves as before.  A row whose clip has ended is IDLE until the next clip moves in (``finish_clips``): its
bank is cut back to its first entry and frozen -- it never appends, is never scored and never lengthens the group's T.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import ops
from .runtime import MAX_CHUNKS


def bank_slots(n_keep: int) -> int:
    """Bank slots per clip of a runtime: a restricted bank holds N + 1 entries between append and eviction; an unbounded one as
    many as the key table has rows."""
    return n_keep + 1 if n_keep < MAX_CHUNKS else MAX_CHUNKS


class MemoryPolicy:
    """Which bank entry to evict (layers/transformer.py:338-411, eval branch).

    Inputs are the per-memory-frame attention mass of layer 0 weighted by the
    foreground probability (already reduced over tokens on the device); the EMA (0.8) with the
    stored score of the same frame index, the UCB bonus 1.5*sqrt(log(sum n)/(n_i+8)) with
    n_0 := T', and the argmin over entries >= 1 are evaluated here in fp32 torch CPU ops,
    the same arithmetic the reference runs.
    """

    def __init__(self):
        self.ema: Dict[int, torch.Tensor] = {}
        self.visits: Dict[int, int] = {}

    def choose(self, scores: torch.Tensor, indexes: List[int]) -> int:
        a = (scores / scores.sum()).clone()
        cur = {indexes[i]: a[i].clone() for i in range(a.shape[0])}
        cur = {k: ((1 - 0.8) * self.ema[k] + 0.8 * v) if k in self.ema else v for k, v in cur.items()}
        self.ema = cur
        for i in range(a.shape[0]):
            a[i] = cur[indexes[i]]
        self.visits = {k: 1 + self.visits.get(k, 0) for k in indexes}
        n = torch.tensor([float(self.visits[k]) for k in indexes[:-1]])
        n[0] = len(n)
        a = a + 1.5 * torch.sqrt(torch.log(n.sum()) / (n + 8))
        rest = a[1:]
        return int(torch.argmin(rest).item()) + 1 if rest.shape[0] > 0 else 1


def device_scores(rt, stream, clips: List[int], T: int, keep: int):
    """Eviction scores of ``clips`` (attention mass of layer 0, [L][T] per clip, weighted by the foreground probability; ids above
    ``keep`` masked) reduced on the device and read back into ``rt.scores_host``; returns the event that says they arrived."""
    s, L = stream.cuda_stream, rt.L
    ops.run([ops.evict_scores(rt.logits[c * rt.M4:(c + 1) * rt.M4], rt.mass[c * L * T:(c + 1) * L * T], rt.scores[c], ldl=16,
                              nc=rt.nc, keep=keep, Hi=rt.H4, Wi=rt.W4, He=rt.H16, We=rt.W16, T=T) for c in clips], s)
    for c in clips:
        ops.copy_async(rt.scores_host[c], rt.scores[c], 4 * T)(s)
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


class BankSchedule:
    """The banks of ``clips`` clips (rows) of one engine.  ``owner`` is the engine: ``frame_step``, ``long_term_mem_gap`` (the defaults
    of rows without a counter / gap of their own), ``cfg`` (bank
    length, NO_LONG_MEMORY), ``policy_every_update`` and ``stream`` are read from it when a decision is taken (callers set the gap
    on a started engine).  The runtime whose ``slots`` / ``free`` / ``S`` the decisions act on is an argument: an engine may
    replace its runtime, the index lists outlive it."""

    def __init__(self, owner, clips: int, score=device_scores):
        self.owner, self.B, self.score = owner, clips, score
        self.restart()

    def restart(self, rt=None):
        """New clips: empty banks, index lists and traces; a pending policy update is discarded."""
        B = self.B
        self.last_mem_step: List[int] = [-1] * B
        self.indexes: List[List[int]] = [[] for _ in range(B)]
        self.policies = [MemoryPolicy() for _ in range(B)]
        self.drop_trace: List[List[int]] = [[] for _ in range(B)]
        self.row_step: List[Optional[int]] = [None] * B    # the row's own frame counter (None: the owner's frame_step)
        self.row_gap: List[Optional[int]] = [None] * B     # the row's own gap (None: the owner's long_term_mem_gap)
        self.idle: set = set()                             # rows whose clip has ended and has not been replaced
        self._pending = None
        self._mass_valid = False
        self._T_at_propagate = 0                         # the group's T: layout of the mass buffer
        self._Tc_at_propagate: List[int] = [0] * B       # each clip's own bank length: what its policy sees
        if rt is not None:
            rt.reset_bank()

    @property
    def n_keep(self) -> int:
        return self.owner.cfg.FORMER_MEM_LEN + self.owner.cfg.LATTER_MEM_LEN

    def _s(self) -> int:
        return self.owner.stream.cuda_stream

    def step_of(self, c: int) -> int:
        """Frame index row ``c`` is at, counted from its clip's frame 0."""
        return self.owner.frame_step if self.row_step[c] is None else self.row_step[c]

    def gap_of(self, c: int) -> int:
        return self.owner.long_term_mem_gap if self.row_gap[c] is None else self.row_gap[c]

    def advance(self):
        """The next frame is propagated: rows with a frame counter of their own move on by one frame (idle rows stay)."""
        for c in range(self.B):
            if self.row_step[c] is not None and c not in self.idle:
                self.row_step[c] += 1

    def long_memories_indexes(self, clip: int) -> List[int]:
        """Frame indexes of the clip's bank entries (aot_engine.py:323, 351); resolves a deferred eviction first."""
        self.resolve()
        return self.indexes[clip]

    # ------------------------------------------------------------------ reference frame (aot_engine.py:318-323)
    @staticmethod
    def restart_banks(rt, clips: Iterable[int], stream: int, append_table: bool = True) -> List[int]:
        """The banks of ``clips`` := one entry each, in the clip's lowest slot (all its slots go back to the free list in ascending
        order first).  Uploads the key table and, for a reference-mode launch that writes the entry, the append table; returns
        the per-clip slot (-1: clip not restarted)."""
        first = [-1] * rt.B
        for c in clips:
            rt.free[c] = sorted(rt.free[c] + rt.slots[c])
            first[c] = rt.free[c].pop(0)
            rt.slots[c] = [first[c]]
        rt.upload_chunks(stream)
        if append_table:
            rt.upload_append_slots(first, stream)
        return first

    def start_reference(self, rt, clips: Optional[Iterable[int]] = None, mem_step: Optional[int] = None,
                        append_table: bool = True) -> List[int]:
        """A reference frame for ``clips`` (default: all): bank := this frame only, policy reset, the long-term schedule restarts
        at ``mem_step`` (default: the frame counter) while ``long_memories_indexes`` keeps growing with the frame counter (the
        reference's quirk, 323).  A pending eviction belongs to the bank that is reset here, but its effect on the index list (the
        reference keeps that list across the reset) and on the policy state still happens first -- on the runtime it was issued
        on, which ``rt`` may have replaced (a frame of another size)."""
        self.resolve()
        clips = list(range(self.B) if clips is None else clips)
        for c in clips:
            step = self.step_of(c)
            self.last_mem_step[c] = step if mem_step is None else mem_step
            self.policies[c] = MemoryPolicy()
            self.indexes[c].append(step)
        return self.restart_banks(rt, clips, self._s(), append_table)

    # ------------------------------------------------------------------ ragged groups: a NEW CLIP per row
    def start_clips(self, rt, rows: Iterable[int], gaps: Iterable[int], append_table: bool = False) -> List[int]:
        """A new clip starts in ``rows`` with the per-row ``gaps``.  Unlike a mid-clip reference frame (start_reference keeps the
        row's index list growing, which is why a later eviction of that clip raises) the row starts over: index list [0], empty
        drop trace, a fresh policy, last long-term update and frame counter at the clip's own frame 0, bank := one entry.  A
        pending eviction is resolved first (it may belong to another row; a finished row's traces were handed out by
        finish_clips).  -> per-row bank slot of the entry (-1: row not started); the caller writes the entry."""
        self.resolve()
        rows = list(rows)
        for c, gap in zip(rows, gaps):
            self.idle.discard(c)
            self.row_step[c], self.row_gap[c] = 0, int(gap)
            self.last_mem_step[c] = 0
            self.policies[c] = MemoryPolicy()
            self.indexes[c] = [0]
            self.drop_trace[c] = []
        return self.restart_banks(rt, rows, self._s(), append_table)

    def finish_clips(self, rt, rows: Iterable[int]) -> List[Tuple[List[int], List[int]]]:
        """The clips of ``rows`` have ended: -> their (long_memories_indexes, drop_trace), a deferred eviction resolved first.  The
        rows are idle from here on; their banks keep the first entry only (a bank the memory read has run on, of the shortest
        length there is), so an idle row never lengthens T."""
        self.resolve()
        rows = list(rows)
        out = [(list(self.indexes[c]), list(self.drop_trace[c])) for c in rows]
        for c in rows:
            self.idle.add(c)
            rt.free[c] = sorted(rt.free[c] + rt.slots[c][1:])
            del rt.slots[c][1:]
        if rows:
            rt.upload_chunks(self._s())
        return out

    # ------------------------------------------------------------------ propagate
    def _will_append(self, c: int) -> bool:
        if c in self.idle or getattr(self.owner.cfg, 'NO_LONG_MEMORY', False):
            return False
        return self.step_of(c) - self.last_mem_step[c] >= self.gap_of(c)

    def begin_propagation(self, rt) -> Tuple[int, bool]:
        """-> (bank size T the launches are built for: the longest bank; whether the attention mass of layer 0 is wanted).  The
        mass (layers/transformer.py:636-643) is only read by the eviction policy, i.e. when the update after this propagation
        appends to some clip's bank (aot_engine.py:338-343) and overflows it (policy_every_update: appends at all): both are
        known now, so the other frames skip the reduction."""
        self.resolve()
        self._Tc_at_propagate = [len(sl) for sl in rt.slots]
        self._T_at_propagate = max(self._Tc_at_propagate)
        self._mass_valid = any(self._will_append(c) and (self.owner.policy_every_update or self._Tc_at_propagate[c] + 1 > self.n_keep)
                               for c in range(self.B))
        return self._T_at_propagate, self._mass_valid

    # ------------------------------------------------------------------ memory update (aot_engine.py:327-369)
    def take_append_slots(self, rt, skip: Iterable[int] = ()) -> List[int]:
        """Per clip the free slot this update appends into, or -1 (no long-term update for it now, or in ``skip``); uploads the
        append table if any clip appends.  The update's launch list runs next, then commit_update."""
        skip = set(skip)
        slots = [-1] * self.B
        for c in range(self.B):
            if self._will_append(c) and c not in skip:
                if not rt.free[c]:
                    raise ops.RmemError(f'clip {c}: the memory bank outgrew the {rt.S} slots of the runtime '
                                        f'(unbounded banks are limited by the {MAX_CHUNKS}-row key table)')
                slots[c] = rt.free[c].pop(0)
        if max(slots) >= 0:
            rt.upload_append_slots(slots, self._s())
        return slots

    def commit_update(self, rt, slots: List[int], keep: int):
        """The entries of take_append_slots are in the bank.  Clips whose bank now overflows (policy_every_update: every clip that
        appended) get their eviction scores reduced and read back asynchronously; the decision is taken in resolve.  The key
        table is uploaded there if a policy update is pending, here otherwise."""
        if max(slots) < 0:
            return
        scored, over = [], set()            # clips whose policy state moves / whose bank overflows
        for c, slot in enumerate(slots):
            if slot >= 0:
                self.last_mem_step[c] = self.step_of(c)
                rt.slots[c].append(slot)
                self.indexes[c].append(self.step_of(c))
                if len(rt.slots[c]) > self.n_keep:
                    over.add(c)
                if c in over or self.owner.policy_every_update:
                    scored.append(c)
        if not scored:
            rt.upload_chunks(self._s())
            return
        if not self._mass_valid:
            raise RuntimeError('long_term_mem_gap / memory length changed between propagation and memory update: '
                               'the attention mass of this frame was not recorded')
        ev = self.score(rt, self.owner.stream, scored, self._T_at_propagate, keep)
        self._pending = (rt, ev, scored, over, list(self._Tc_at_propagate))

    def resolve(self):
        """Finish a deferred policy update: wait for the score readback (normally long done; the reference syncs here too,
        transformer.py:353), run the policy on the host (353-411), drop the evicted entry from the slot order and the index list
        and upload the new key table -- on the runtime the readback was issued on."""
        if self._pending is None:
            return
        rt, ev, scored, over, tc = self._pending
        self._pending = None
        ev.synchronize()
        for c in scored:
            drop = self.policies[c].choose(rt.scores_host[c, :tc[c]].clone(), self.indexes[c])
            if c not in over:                 # policy_every_update: the scores moved, nothing is dropped yet
                continue
            self.drop_trace[c].append(drop)
            rt.free[c].append(rt.slots[c].pop(drop))
            del self.indexes[c][drop]
        rt.upload_chunks(self._s())
