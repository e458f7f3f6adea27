"""Clip-parallel driver: many clips in flight per GPU, one process per GPU.

Mirrors the reference's evaluation protocol (managers/evaluator.py:330-335, 385-441, 509-523:
per-sequence gap = max(round(n/30), 5), reference frame, then propagate -> argmax -> update per
frame) and its multi-GPU scheme (tools/eval.py:137-143, evaluator.py:276-295: one worker per GPU
draining a queue of sequences; no collective on the data path, one final gather of statistics).
Frames inside a clip are strictly sequential (short-term memory recurrence + mask feedback), so
a GPU is filled by interleaving independent clips: each clip owns an engine, a HIP stream and its
hipGraphs; the host only enqueues.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib, ops
from .frame_feed import FrameFeed
from .jpeg import JpegClip


def clip_gap(n: int) -> int:
    """The long_term_mem_gap of a clip of n frames (managers/evaluator.py:330-335)."""
    return max(int(round(n / 30)), 5)


def shard_clips(num_clips: int, rank: int, world: int, lengths: Optional[Sequence[int]] = None) -> List[int]:
    """Static longest-first assignment of clip ids to ranks (the reference pops a shared queue; with
    equal hardware a greedy longest-first split gives the same balance without a host-side queue)."""
    ids = list(range(num_clips))
    if lengths is not None:
        ids.sort(key=lambda i: (-lengths[i], i))
    loads = [0] * world
    mine: List[int] = []
    for i in ids:
        r = min(range(world), key=lambda j: (loads[j], j))
        loads[r] += lengths[i] if lengths is not None else 1
        if r == rank:
            mine.append(i)
    return mine


def group_units(lengths: Sequence[int], group: int) -> List[List[int]]:
    """Work units of a clip list for engines that advance ``group`` clips in lockstep: clips of EQUAL length (equal length
    => equal gap, managers/evaluator.py:330-335) are bundled ``group`` at a time, longest first; a length whose clip count is
    not a multiple of ``group`` leaves one shorter unit (run by a smaller group or the per-clip engine)."""
    by_len = {}
    for i, n in enumerate(lengths):
        by_len.setdefault(int(n), []).append(i)
    units = []
    for n in sorted(by_len, reverse=True):
        ids = by_len[n]
        units += [ids[k:k + group] for k in range(0, len(ids), group)]
    return units


class ClipFeeder:
    """Hands the work units of a job's clip list to this rank -- the counterpart of the reference's sequence queue
    (tools/eval.py:137-143 spawns one worker per GPU; managers/evaluator.py:276-295 has every worker pop sequences from one
    shared mp.Queue until it is empty).  No data-path collective is involved in either mode:

      'queue'  (default for world > 1) a job-wide ticket counter on the process group's TCPStore (``store.add``): whichever
               rank has a free slot takes the next unit, longest first, so a slow rank or a skewed list costs at most one unit
               of tail (host-side work stealing; one ~50 us store round trip per CLIP, never per frame);
      'static' the longest-first greedy split of ``shard_clips`` computed identically on every rank (no store traffic).

    ``cyclic``: after the last unit the list starts over (bench.py measures a fixed-length window of a long job).

    ``store``: any c10d store shared by the ranks (bench.py passes the TCPStore its process group was initialised with); the
    feeder works inside its own PrefixStore namespace, ``<key>/<n>`` for the n-th feeder this process created -- every rank
    creates its feeders in the same order, so the n-th feeders of all ranks share one ticket counter that starts at zero, and
    a second job in the same process group does not inherit the first one's tickets."""

    _instances = 0

    def __init__(self, lengths: Sequence[int], rank: int = 0, world: int = 1, group: int = 1, mode: Optional[str] = None,
                 store=None, cyclic: bool = False, key: str = 'rmem_clip_queue'):
        self.lengths = [int(n) for n in lengths]
        self.units = group_units(self.lengths, group)
        self.rank, self.world, self.cyclic = rank, world, cyclic
        self.key = f'{key}/{ClipFeeder._instances}'
        ClipFeeder._instances += 1
        self.mode = mode or ('queue' if world > 1 else 'static')
        if self.mode not in ('queue', 'static'):
            raise ValueError(f'ClipFeeder mode {self.mode!r}: expected "queue" or "static"')
        if self.mode == 'queue' and world > 1:
            if store is None:
                raise ValueError('ClipFeeder: the job-wide queue needs the c10d store the ranks share (store=...)')
            import torch.distributed as dist
            self.store = dist.PrefixStore(self.key, store)
        else:
            self.store = None
        unit_len = [self.lengths[u[0]] * len(u) for u in self.units]
        self._mine = shard_clips(len(self.units), rank, world, unit_len)      # static order (also the world == 1 order)
        self._taken = 0
        self.history: List[int] = []         # unit indexes this rank ran, in order

    def next_unit(self) -> Optional[List[int]]:
        """Clip ids of the next unit for this rank, or None when the list is drained."""
        n = len(self.units)
        if self.store is not None:
            t = int(self.store.add('ticket', 1)) - 1                  # job-wide ticket
            if t >= n and not self.cyclic:
                return None
            u = t % n
        else:
            if not self._mine or (self._taken >= len(self._mine) and not self.cyclic):
                return None
            u = self._mine[self._taken % len(self._mine)]
            self._taken += 1
        self.history.append(u)
        return self.units[u]


def open_job_store(rank: int, world: int):
    """The c10d store of this job, opened explicitly from MASTER_ADDR / MASTER_PORT (``env://`` rendezvous: under
    torch.distributed.run it is a client of the launcher's TCPStore, otherwise rank 0 hosts it).  bench.py hands the SAME store
    to ``init_process_group(store=...)`` and to ClipFeeder, so nothing reaches into the process group's internals."""
    import torch.distributed as dist
    store, _, _ = next(iter(dist.rendezvous('env://', rank, world)))
    return store


DRAIN = 1 << 62


def pump(slots: Sequence, start_fn, steps: int, frames_per_step: int = 1) -> int:
    """Advance the slots round-robin until ``steps`` propagated frames have been enqueued (one slot step = ``frames_per_step``
    frames: the clips of a group move together).  A slot whose clip has ended takes the next unit of the job through
    ``start_fn(slot)`` (reference frames: executed, not counted); start_fn returns False when the list is drained, the slot then
    idles.  Returns the frames actually enqueued (< steps only if every slot ran dry: ``steps = DRAIN`` runs the job to its end,
    bench.py --drain).  Host-side only: nothing here waits for the GPU."""
    done, j, idle = 0, 0, 0
    n = len(slots)
    while done < steps and idle < n:
        s = slots[j % n]
        j += 1
        if s.done and start_fn(s) is False:
            idle += 1
            continue
        if s.done:                      # a unit of single-frame clips: nothing to propagate
            idle = 0
            continue
        idle = 0
        s.step()
        done += frames_per_step
    return done


def gather_stats(frames: float, seconds: float, checksum: float, dist, rank: int, world: int, device):
    """The one exchange of the clip-parallel design (reference: info_queue, managers/evaluator.py:589-613):
    every rank sends (frames, seconds, checksum) to rank 0, which returns (sum frames, max seconds, sum checksum)."""
    stats = torch.tensor([frames, seconds, checksum], dtype=torch.float64, device=device)
    if dist is None or world == 1:
        return float(stats[0]), float(stats[1]), float(stats[2])
    gathered = [torch.zeros_like(stats) for _ in range(world)] if rank == 0 else None
    dist.gather(stats, gathered, dst=0)
    if rank != 0:
        return None
    return (sum(float(g[0]) for g in gathered), max(float(g[1]) for g in gathered), sum(float(g[2]) for g in gathered))


class ClipSlot:
    """One clip in flight: an engine, its frames on the device, its output label buffer."""

    def __init__(self, engine, out_hw, device, lookahead: int = 1):
        self.engine = engine
        self.lookahead = lookahead          # > 1: the encoder runs this many frames ahead, one launch per layer for all of them
        self.labels: Optional[torch.Tensor] = None
        self.cur_label = torch.zeros(out_hw[0], out_hw[1], dtype=torch.uint8, device=device)   # fixed address (graph-captured)
        self.out_hw = out_hw
        self.device = device
        self.feed = FrameFeed(device, lookahead=lookahead)
        self.frames = None
        self.cursor = 0
        self.done = True
        self.frames_encoded = 0             # frames that went through the encoder (reference frames + look-ahead batches)

    def start(self, frames: torch.Tensor, first_mask: torch.Tensor, num_objs: int):
        """frames [n,3,H,W] fp32 device at network size, or decoded uint8 RGB [n,Hs,Ws,3] in PINNED HOST memory (then every
        frame crosses PCIe as uint8 and is resized + normalised on the device, rmem_ingest_rgb8), or a JpegClip (only the
        compressed frames cross PCIe; they are decoded on the device into the same uint8 rows; start() raises RmemError if a
        frame of the PREVIOUS JpegClip did not decode cleanly, check_frames() checks the current one);
        first_mask [1,1,H,W] at network size."""
        self.check_frames()
        n = frames.shape[0]
        self.frames = frames
        self.host_u8 = frames.dtype == torch.uint8
        if self.labels is None or self.labels.shape[0] < n:
            self.labels = torch.zeros(n, self.out_hw[0], self.out_hw[1], dtype=torch.uint8, device=self.device)
        eng = self.engine
        eng.restart_engine()
        eng.long_term_mem_gap = clip_gap(n)
        if self.host_u8:
            self.feed.check_pinned(frames)
            self._first = self.feed.rows('first', (1, 3, int(first_mask.shape[-2]), int(first_mask.shape[-1])))
            cur = torch.cuda.current_stream(self.device)
            # the engine's own stream may still be running the previous clip's last frames, which read the staging rows / _first:
            # order this clip's first-frame copy + ingest behind them (a device-side wait, no host stall)
            for e in eng.aot_engines + getattr(eng, '_pool', []):
                cur.wait_stream(e.stream)
            self._ingest_group(0, 1, self._first, cur.cuda_stream)
            cur.synchronize()        # once per clip: the engine works on its own stream
            eng.add_reference_frame(self._first, first_mask, obj_nums=[num_objs], frame_step=0)
        else:
            eng.add_reference_frame(frames[0:1], first_mask, obj_nums=[num_objs], frame_step=0)
        self.frames_encoded += 1
        self.cursor = 1
        self.done = n <= 1

    def check_frames(self):
        """Once per JPEG clip: wait for the clip's work and raise RmemError if one of its frames did not decode cleanly (a
        corrupt entropy-coded segment behind valid headers).  A no-op for other frame sources."""
        if isinstance(self.frames, JpegClip):
            self.engine.synchronize()
            torch.cuda.current_stream(self.device).synchronize()
            self.frames.check(self.device)

    def _ingest_group(self, i: int, m: int, dst: torch.Tensor, stream: int):
        """Host -> device copy (or decode) of uint8 frames i .. i+m-1 and their resize + normalise into dst[0:m] on ``stream``."""
        stage = self.feed.stage(max(self.lookahead, 1), int(self.frames.shape[1]), int(self.frames.shape[2]))
        self.feed.ingest([(self.frames, i, m, stage, dst)], stream)

    def step(self):
        """Propagate one frame and update the memory with the predicted labels (all asynchronous)."""
        i = self.cursor
        s = self.engine.aot_engines[0].stream.cuda_stream          # the clip's stream
        if self.lookahead > 1:
            e = (i - 1) % self.lookahead
            if e == 0:
                m = min(self.lookahead, self.frames.shape[0] - i)
                self.frames_encoded += m
                if self.host_u8:
                    self._ingest_group(i, m, self.engine.encode_inputs(self.lookahead), s)
                    self.engine.encode_ahead(None, self.lookahead)
                else:
                    self.engine.encode_ahead(self.frames[i:i + self.lookahead], self.lookahead)
            self.engine.propagate_to_label(None, self.cur_label, enc_slot=e)
        elif self.host_u8:
            self.frames_encoded += 1
            self._ingest_group(i, 1, self._first, s)
            self.engine.propagate_to_label(self._first, self.cur_label)
        else:
            self.frames_encoded += 1
            self.engine.propagate_to_label(self.frames[i:i + 1], self.cur_label)
        self.engine.update_memory_from_label_u8(self.cur_label)
        # the clip's delivered masks stay on the device
        ops.copy_async(self.labels[i], self.cur_label, self.cur_label.numel())(s)
        self.cursor += 1
        self.done = self.cursor >= self.frames.shape[0]


class GroupSlot:
    """B clips of equal length in flight on one GroupEngine (networks/engines/group_engine.py): same protocol as ClipSlot, one
    launch per layer for the whole group.  With an encoder look-ahead of n frames the frames are encoded in batches of n per
    clip: batch k + 1 is copied in and encoded on the engine's side stream while the frames of batch k are propagated (two
    look-ahead buffers, alternating; look-ahead slot = buffer * n + frame).
    labels: uint8 [B, n, Ho, Wo] on the device, labels[c, i] = the prediction of frame i of clip c (row 0 stays zero: frame 0 is the
    given annotation).  Once the engine has been synchronised a clip is scored where it lies:
    evaluator.score_clip(slot.labels[c, :n], gt_stack) -> J, F, J&F, decay, tail J; and its masks leave as palette PNGs encoded
    on the device: png.encode_label_stack(slot.labels[c, 1:n]) -> one PNG file per frame (evaluator.save_masks writes them).

    FLIP TESTING: on a GroupEngine(flip_tta=True) of B = 2P rows the slot takes P clips and delivers labels [P, n, Ho, Wo]; rows
    P..2P-1 are the clips' horizontally mirrored twins, which the slot makes on the device: the twins' frames are mirrored look-ahead
    batch by look-ahead batch on the encoder stream (into staging rows per look-ahead buffer for fp32 device frames, whose
    lifetime the encoder events cover; next to the ingested frames in the encoder's input for uint8 / JPEG sources) -- a frame
    crosses PCIe once, a JPEG is decoded once, no mirrored clip is kept; the twins' first masks are the mirrored network-size
    masks (resized, THEN mirrored: evaluator.py:319-323); cur_label stays [2P, Ho, Wo] with the merged label in row p and its
    mirror in row P + p (the engine's fused pair kernel writes both), so the twins' memory updates take it as it is."""

    def __init__(self, engine, out_hw, device):
        self.engine = engine
        self.B = engine.B
        self.flip = bool(getattr(engine, 'flip_tta', False))
        self.clips = self.B // 2 if self.flip else self.B        # clips the caller hands in (rows beyond them are mirrored twins)
        self.out_hw = out_hw
        self.device = device
        self.feed = FrameFeed(device, self.B, self.clips, engine.lookahead, self.flip)
        self.cur_label = torch.zeros(self.B, out_hw[0], out_hw[1], dtype=torch.uint8, device=device)   # fixed address (graph-captured)
        self.labels: Optional[torch.Tensor] = None
        self.frames = None
        self._frames_by_pointer = False
        self.cursor = 0
        self.done = True
        self.frames_encoded = 0             # frames that went through the encoder (reference frames + look-ahead batches)

    def start(self, frames: Sequence[torch.Tensor], first_masks: Sequence[torch.Tensor], num_objs: int, new_objects=None):
        """frames: B tensors [n, 3, H, W] fp32 device (equal n), or B uint8 [n, Hs, Ws, 3] tensors in PINNED HOST memory (every
        frame then crosses PCIe as uint8 and is resized + normalised on the device), or B JpegClips (decoded on the device into
        the same uint8 staging rows, look-ahead group by look-ahead group; start() raises RmemError if a frame of the PREVIOUS
        clips did not decode cleanly, check_frames() checks the current ones); first_masks: B tensors [1, 1, H, W] at the
        network size.  new_objects: {clip index: (frame index, uint8 [Ho, Wo] device map: the new object's label on its pixels, 0
        elsewhere)} -- the evaluator's protocol for an object that appears mid-clip (managers/evaluator.py:484-508): the frame is
        propagated, the new label is laid over the prediction and the frame is re-added as a reference frame for that clip."""
        assert len(frames) == self.clips and len({int(f.shape[0]) for f in frames}) == 1
        n = int(frames[0].shape[0])
        self.check_frames()                       # JPEG clips: waits for their decodes, so they can be let go of
        if self._frames_by_pointer:
            self.engine.enc_stream.synchronize()  # queued encoder launches read the previous clips' frames in place: let go of them after
        self.frames = list(frames)
        self.host_u8 = frames[0].dtype == torch.uint8
        self.new_objects = dict(new_objects or {})
        if self.new_objects and self.host_u8:
            raise ValueError('new_objects: frames must be fp32 device tensors at the network size')
        if self.labels is None or self.labels.shape[1] < n:
            self.labels = torch.zeros(self.clips, n, self.out_hw[0], self.out_hw[1], dtype=torch.uint8, device=self.device)
        eng = self.engine
        self._frames_by_pointer = not self.host_u8 and eng.lookahead > 1
        eng.restart_engine()
        eng.long_term_mem_gap = clip_gap(n)
        H, W = int(first_masks[0].shape[-2]), int(first_masks[0].shape[-1])
        with torch.cuda.stream(eng.stream):
            s = eng.stream.cuda_stream
            if self.host_u8:
                for f in frames:
                    self.feed.check_pinned(f)
                self._first = self.feed.rows('first', (self.B, 3, H, W))
                imgs = self._ingest_frame(0)
            else:
                imgs = torch.cat([f[0:1] for f in frames] * (2 if self.flip else 1), 0)
            masks = torch.cat([m.reshape(1, 1, m.shape[-2], m.shape[-1]).float() for m in first_masks] * (2 if self.flip else 1), 0)
            if self.flip:                                       # the twins' reference frames and first masks
                self.feed.mirror(imgs[:self.clips], imgs[self.clips:], s)
                self.feed.mirror(masks[:self.clips], masks[self.clips:], s)
        eng.add_reference_frames(imgs, masks, num_objs)
        self.frames_encoded += self.B
        self.cursor = 1
        self.done = n <= 1
        if eng.lookahead > 1 and n > 1:
            self._kick_encoder(0, 1)                            # frames 1 .. lookahead: batch 0

    def check_frames(self):
        """Once per group of JPEG clips: wait for the group's work and raise RmemError if a frame did not decode cleanly.  A
        no-op for other frame sources."""
        clips = [f for f in (self.frames or []) if isinstance(f, JpegClip)]
        if clips:
            self.engine.synchronize()
            torch.cuda.current_stream(self.device).synchronize()
            for c in clips:
                c.check(self.device)

    def _kick_encoder(self, buf: int, i: int):
        """Encode frames i .. i + lookahead - 1 of every clip into look-ahead buffer ``buf`` on the engine's side stream."""
        self.frames_encoded += self.B * self.feed.kick(self.engine, buf, {c: (f, i, None) for c, f in enumerate(self.frames)})

    def _ingest_frame(self, i: int) -> torch.Tensor:
        """uint8 sources: frame i of every clip into rows 0..P-1 of _first on the engine's main stream -> _first"""
        stage = self.feed.stage(self.clips, int(self.frames[0].shape[1]), int(self.frames[0].shape[2]))
        self.feed.ingest([(f, i, 1, stage[c:], self._first[c:]) for c, f in enumerate(self.frames)], self.engine.stream.cuda_stream)
        return self._first

    def step(self, feed: Optional[torch.Tensor] = None):
        """Propagate frame ``cursor`` of every clip, deliver its labels and update the memories.  feed: uint8 [clips, Ho, Wo] device
        labels that go into the memory update INSTEAD of the prediction (the delivered labels stay the prediction): given masks,
        e.g. the reference's own in the parity tests, so that every frame is an independent comparison (flip testing: the twins
        are fed the mirror)."""
        self._propagate_step()
        inject = self._settle_labels(feed)
        self._update_memories(inject)
        if feed is None:
            self._deliver()
        self._advance()

    # the parts of step(): MultiScaleGroupSlot runs them engine by engine around its merge across engines
    def _propagate_step(self, to_logits: bool = False):
        """Frame ``cursor`` of every row through the engine into cur_label -- or, to_logits, as far as the engine's logits (-> the
        event behind them); before that the look-ahead encoder of the next batch is kicked where one is due."""
        eng, B, i, P = self.engine, self.B, self.cursor, self.clips
        la = eng.lookahead
        s = eng.stream.cuda_stream
        if la > 1:
            b, e = divmod(i - 1, la)
            if e == 0 and i + la < self.frames[0].shape[0]:
                self._kick_encoder((b + 1) % 2, i + la)         # the NEXT batch, on the side stream, beside this batch's frames
            if to_logits:
                return eng.propagate_to_logits(enc_slot=(b % 2) * la + e)
            eng.propagate_to_labels(self.cur_label, enc_slot=(b % 2) * la + e)
        else:
            self.frames_encoded += B
            if self.host_u8:
                imgs = self._ingest_frame(i)
            else:
                with torch.cuda.stream(eng.stream):
                    imgs = torch.cat([f[i:i + 1] for f in self.frames] * (B // P), 0)
            if self.flip:
                self.feed.mirror(imgs[:P], imgs[P:], s)
            if to_logits:
                return eng.propagate_to_logits(imgs=imgs)
            eng.propagate_to_labels(self.cur_label, imgs=imgs)

    def _deliver(self):
        """cur_label's clip rows -> frame ``cursor`` of every clip's label stack: one pitched copy on the engine's stream"""
        nb = self.cur_label[0].numel()
        ops.copy2d_async(self.labels.view(-1)[self.cursor * nb:], self.labels.shape[1] * nb, self.cur_label, nb, nb, self.clips)(
            self.engine.stream.cuda_stream)

    def _settle_labels(self, feed: Optional[torch.Tensor]) -> List[int]:
        """cur_label holds the prediction -> what the memories continue from: the fed labels (the prediction is delivered first),
        new objects laid over it.  -> the clips that take a new object at this frame."""
        eng, i, P = self.engine, self.cursor, self.clips
        s = eng.stream.cuda_stream
        inject = [c for c, (fi, _) in self.new_objects.items() if fi == i]
        if feed is not None:                          # deliver the prediction, then continue from the given labels
            self._deliver()
            ops.copy_async(self.cur_label, feed.contiguous(), P * self.cur_label[0].numel())(s)
            if self.flip:
                with torch.cuda.stream(eng.stream):
                    self.cur_label[P:].copy_(self.cur_label[:P].flip(-1))
        if inject:
            with torch.cuda.stream(eng.stream):
                for c in inject:                      # the new object's label over the prediction (evaluator.py:484-497)
                    new = self.new_objects[c][1]
                    self.cur_label[c].copy_(torch.where(new > 0, new, self.cur_label[c]))
                    if self.flip:                     # and its mirror over the twin's row, which holds the mirrored prediction
                        self.cur_label[P + c].copy_(self.cur_label[c].flip(-1))
        return inject

    def _update_memories(self, inject: List[int]):
        """The engine's memory update from cur_label; the clips of ``inject`` restart from this frame as their reference frame."""
        eng, i, P = self.engine, self.cursor, self.clips
        s = eng.stream.cuda_stream
        rows = inject + [P + c for c in inject] if self.flip else inject
        eng.update_from_labels(self.cur_label, skip=rows)
        for c in inject:
            eng.add_reference_frame_for(c, self.frames[c][i], self.cur_label[c])
            if self.flip:                             # the twin is re-initialised from the mirrored frame and the mirrored label
                twin = self.feed.rows('twin_ref', self.frames[c][i].shape)
                self.feed.mirror(self.frames[c][i], twin, s)
                eng.add_reference_frame_for(P + c, twin, self.cur_label[P + c])

    def _advance(self):
        self.cursor += 1
        self.done = self.cursor >= self.frames[0].shape[0]


class MultiScaleGroupSlot:
    """MULTI-SCALE TESTING (TEST_MULTISCALE, managers/evaluator.py:342-355, 427-441) of P clips of equal length at group speed: one
    GroupEngine per scale, each a plain group of P rows or (flip testing) a flip group of 2P rows at its own network size, with its
    own streams, graphs, banks and look-ahead; what GroupSlot does per engine (reference frames, look-ahead batches, twin
    mirroring, new objects) is done by one inner GroupSlot per engine.  The scales are coupled at one place per frame: ONE label
    buffer cur_label [B, Ho, Wo] at a fixed address, written by ops.logits_post_ms_merge from the 1/4-resolution logits of every
    engine (members in the evaluator's order: scale outer, flip inner; the twins' logits are rows P.. of their engine's buffer),
    rows P.. with the mirror.  Every engine updates its memory from that buffer: its id-embed kernel resizes to its own network
    size, the twins from the mirrored rows (mirror, THEN resize).  labels: uint8 [P, n, Ho, Wo], as GroupSlot's.

    ORDER of a step.  Every engine propagates to its logits on its own stream and records an event; engine 0's stream waits for
    the other engines' events, merges, delivers, applies fed labels and new objects and records "label ready"; the other streams
    wait for that; every engine updates (and restarts injected rows) on its own stream.  No further event is needed: an engine's
    ``rt.logits`` is rewritten only by its next propagation, which sits behind its update on the same stream, which sits behind
    the merge that read them; cur_label is rewritten only by the next merge, which sits behind every engine's next propagation
    and so behind every update that read it.

    Not taken here (the single-scale slots do): pinned uint8 frames, JpegClips, ragged rows (RaggedGroupSlot)."""

    def __init__(self, engines, out_hw, device):
        engines = list(engines)
        if not engines:
            raise ValueError('MultiScaleGroupSlot: one GroupEngine per scale, at least one')
        for e in engines:
            if isinstance(e, (RaggedGroupSlot, GroupSlot)) or not hasattr(e, 'propagate_to_logits'):
                raise ValueError('MultiScaleGroupSlot takes GroupEngines, one per scale; it does not run on a RaggedGroupSlot (ragged '
                                 'rows stay single-scale)')
        e0 = engines[0]
        for k, e in enumerate(engines[1:], 1):
            for attr, name in (('B', 'rows'), ('flip_tta', 'flip_tta'), ('lookahead', 'lookahead'), ('device', 'device')):
                if getattr(e, attr) != getattr(e0, attr):
                    raise ValueError(f'MultiScaleGroupSlot: engine {k} differs from engine 0 in {name} '
                                     f'({getattr(e, attr)} against {getattr(e0, attr)})')
        self.flip = bool(e0.flip_tta)
        members = len(engines) * (2 if self.flip else 1)
        if members > 8:
            raise ValueError(f'MultiScaleGroupSlot: {len(engines)} scales{" x flip" if self.flip else ""} make {members} members, '
                             'at most 8 are merged')
        self.engines = engines
        self.B = e0.B
        self.clips = self.B // 2 if self.flip else self.B
        self.out_hw = out_hw
        self.device = device
        self.slots = [GroupSlot(e, out_hw, device) for e in engines]
        self.cur_label = self.slots[0].cur_label              # fixed address; ONE buffer for every engine
        for sl in self.slots[1:]:
            sl.cur_label = self.cur_label
        self._ready = None
        self._first = [None] * len(engines)
        self._merge = (None, None)

    labels = property(lambda self: self.slots[0].labels)
    cursor = property(lambda self: self.slots[0].cursor)
    done = property(lambda self: self.slots[0].done)
    frames_encoded = property(lambda self: sum(sl.frames_encoded for sl in self.slots))

    def start(self, frames, first_labels, num_objs: int, new_objects=None):
        """frames[s][c]: fp32 device tensors [n, 3, H_s, W_s], scale s at engine s's network size, equal n; first_labels[c]: fp32
        [1, 1, Ho, Wo] at the OUTPUT size -- resized to every scale's network size on the device (nearest,
        rmem_resize_nearest_flip_f32) and THEN mirrored for the twins, as SequenceEvaluator does.  new_objects: as GroupSlot.start
        (maps at the output size; every engine restarts that clip's rows from its own scale's frame)."""
        P, S = self.clips, len(self.engines)
        if len(frames) != S:
            raise ValueError(f'MultiScaleGroupSlot.start: frames holds one list of clips per scale ({S} scales, got {len(frames)})')
        for fs in frames:
            if isinstance(fs, torch.Tensor) or len(fs) != P:
                raise ValueError(f'MultiScaleGroupSlot.start: every scale takes {P} clips')
            for f in fs:
                if isinstance(f, JpegClip):
                    raise ValueError('MultiScaleGroupSlot: JpegClip sources are not taken (use GroupSlot per scale, or decode first)')
                if f.dtype == torch.uint8:
                    raise ValueError('MultiScaleGroupSlot: pinned uint8 frames are not taken; frames are fp32 device tensors at '
                                     'each scale\'s network size')
        if len({int(f.shape[0]) for fs in frames for f in fs}) != 1:
            raise ValueError('MultiScaleGroupSlot.start: every clip at every scale has the same number of frames')
        if len(first_labels) != P or any(tuple(m.shape[-2:]) != tuple(self.out_hw) for m in first_labels):
            raise ValueError(f'MultiScaleGroupSlot.start: {P} first labels [1, 1, {self.out_hw[0]}, {self.out_hw[1]}] at the output size')
        # held until the next start: the engines' streams read them
        self._first_src = [m.reshape(1, 1, *self.out_hw).float().contiguous() for m in first_labels]
        cur = torch.cuda.current_stream(self.device)
        for k, (eng, sl, fs) in enumerate(zip(self.engines, self.slots, frames)):
            H, W = int(fs[0].shape[-2]), int(fs[0].shape[-1])
            if any(tuple(f.shape[-2:]) != (H, W) for f in fs):
                raise ValueError(f'MultiScaleGroupSlot.start: scale {k}: its clips are not at one network size')
            eng.stream.wait_stream(cur)                   # the first labels come from the caller's stream
            with torch.cuda.stream(eng.stream):
                if self._first[k] is None or tuple(self._first[k].shape[-2:]) != (H, W):
                    self._first[k] = torch.empty(P, 1, 1, H, W, dtype=torch.float32, device=self.device)
                ops.run([ops.resize_nearest_flip(m, self._first[k][c], flip=False) for c, m in enumerate(self._first_src)], eng.stream.cuda_stream)
            if k:
                sl.labels = self.slots[0].labels          # delivered by engine 0's slot only: no second stack
            sl.start(fs, list(self._first[k]), num_objs, new_objects=new_objects)

    def _merge_op(self):
        """the merge across engines, rebuilt when an engine got a new runtime (its logits moved)"""
        P = self.clips
        key = tuple(e.rt.logits.data_ptr() for e in self.engines)
        if self._merge[0] != key:
            members = []
            for e in self.engines:
                rt = e.rt
                members.append((rt.logits, rt.H4, rt.W4, False))
                if self.flip:
                    members.append((rt.logits[P * rt.H4 * rt.W4:], rt.H4, rt.W4, True))
            e0 = self.engines[0]
            if any((e.rt.nc, e.obj_nums[0], e.align_corners) != (e0.rt.nc, e0.obj_nums[0], e0.align_corners) for e in self.engines):
                raise ValueError('MultiScaleGroupSlot: the engines do not share classes, kept ids and align_corners (one model)')
            op = ops.logits_post_ms_merge(members, e0.rt.nc, e0.obj_nums[0], self.out_hw[0], self.out_hw[1], e0.align_corners,
                                          self.cur_label, self.cur_label[P:] if self.flip else None, P=P)
            self._merge = (key, op)
        return self._merge[1]

    def step(self, feed: Optional[torch.Tensor] = None):
        """GroupSlot.step across the scales (the class docstring has the order).  feed: uint8 [P, Ho, Wo], as GroupSlot.step."""
        lead, s0 = self.slots[0], self.engines[0].stream
        events = [sl._propagate_step(to_logits=True) for sl in self.slots]
        for ev in events[1:]:
            s0.wait_event(ev)
        ops.run(self._merge_op(), s0.cuda_stream)
        inject = lead._settle_labels(feed)
        if feed is None:
            lead._deliver()
        if self._ready is None:
            self._ready = torch.cuda.Event()
        self._ready.record(s0)
        for e in self.engines[1:]:
            e.stream.wait_event(self._ready)
        for sl in self.slots:
            sl._update_memories(inject)
            sl._advance()

    def synchronize(self):
        for e in self.engines:
            e.synchronize()


class FinishedClip(NamedTuple):
    """A clip a RaggedGroupSlot has finished: labels uint8 [n, Ho, Wo] on the device (row 0 zero), ``event`` recorded on the engine's
    stream behind the clip's last delivery (a consumer stream waits on it, then scores / saves the stack while the group runs on),
    and the clip's bank traces."""
    clip_id: object
    labels: torch.Tensor
    event: object
    long_memories_indexes: List[int]
    drop_trace: List[int]
    twin_traces: Optional[tuple] = None        # flip testing: (long_memories_indexes, drop_trace) of the mirrored twin's row


class _RaggedClip:
    __slots__ = ('id', 'frames', 'mask', 'new_objects', 'gap', 'n', 'labels', 'host_u8', 'ready')


class _Row:
    __slots__ = ('clip', 'i', 'live')

    def __init__(self):
        self.clip, self.i, self.live = None, 0, False


class RaggedGroupSlot:
    """Clips of ANY length in flight on one GroupEngine: continuous batching for clip groups.  The group is a set of rows; each row
    runs its own clip at its own frame index with its own gap, and when a row's clip ends the next queued clip moves into that row
    (GroupEngine.start_clips: reference frame through the one-clip side runtime, fresh bank schedule for the row) while the other
    rows keep going.  Same protocol per clip as GroupSlot; every clip owns its label stack [n, Ho, Wo] (allocated at submit, row 0
    zero) and is handed out as a FinishedClip when its last frame has been enqueued.

    Look-ahead n > 1: rows are re-assigned at look-ahead batch boundaries.  When batch k + 1 is kicked (at the first step of batch
    k) the slot knows which rows end inside batch k and puts frames 1..n of the next queued clips into those rows of batch k + 1;
    their frame 0 goes through the row-start path at the boundary.  A row whose clip ends mid-batch idles for at most n - 1 steps
    (route mode idle: its label row is zeroed, nothing is delivered; its bank is frozen at one entry).  Look-ahead 1: a row is
    refilled before the next step.  Per step the labels of all rows are routed by ONE launch (ops.LabelRoutes, rmem_route_labels):
    delivery into each clip's stack, a new object's overlay, fed labels, the mirror into a flip twin.

    Frame sources: fp32 device frames at the network size, or uint8 frames in pinned host memory (staged and ingested by the
    slot's FrameFeed, as GroupSlot's).  All clips of a slot share the network size and the output size.  With GroupEngine(flip_tta=True) the slot takes
    B / 2 rows of clips and makes their mirrored twins itself (frames and masks resized, THEN mirrored).

    Counters: row_steps_live / row_steps_idle (rows that propagated a frame of a clip / did not, per step), refills (clips that moved
    into a row another clip had run in), frames_encoded (as in GroupSlot: every row of the group per encoded frame index)."""

    def __init__(self, engine, out_hw, device):
        self.engine = engine
        self.B = engine.B
        self.flip = bool(getattr(engine, 'flip_tta', False))
        self.clips = self.B // 2 if self.flip else self.B
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.device = device
        self.feed = FrameFeed(device, self.B, self.clips, engine.lookahead, self.flip)
        self._queue: List[_RaggedClip] = []
        self._trivial: List[_RaggedClip] = []          # single-frame clips: nothing to propagate
        self._rows = [_Row() for _ in range(self.clips)]
        self._net_hw = None
        self._src_hw = None                            # uint8 sources: their frame size
        self._started = False
        self._k, self._e = 0, 0                        # look-ahead batch counter, frame inside the batch
        self._plan = None                              # {row: (clip, first frame, is new)} of the batch kicked ahead
        self._retired = []                             # (events, clip): frames queued launches may still read in place
        self.cur_label = None
        self.row_steps_live = self.row_steps_idle = self.refills = self.frames_encoded = 0

    # ------------------------------------------------------------------ queue
    def submit(self, clip_id, frames, first_mask, new_objects=None, gap: Optional[int] = None):
        """Queue a clip: frames fp32 [n, 3, H, W] on the device at the network size (work that produces them must have been enqueued
        on the current stream before this call: the engine's streams wait for an event recorded here), or uint8 [n, Hs, Ws, 3] in
        pinned host memory;
        first_mask [1, 1, H, W] at the network size; new_objects {frame index: uint8 [Ho, Wo] device map} (or one (frame index, map)
        pair); gap: the clip's long_term_mem_gap, default max(round(n / 30), 5) (evaluator.py:330-335)."""
        if isinstance(frames, JpegClip):
            raise ValueError(f'RaggedGroupSlot: clip {clip_id!r} is a JpegClip; JPEG sources are out of scope for ragged groups '
                             '(decode the clip first, or run it on GroupSlot / ClipSlot)')
        c = _RaggedClip()
        c.id, c.frames, c.n = clip_id, frames, int(frames.shape[0])
        c.host_u8 = frames.dtype == torch.uint8
        hw = (int(first_mask.shape[-2]), int(first_mask.shape[-1]))
        if not c.host_u8 and tuple(frames.shape[1:]) != (3,) + hw:
            raise ValueError(f'RaggedGroupSlot: clip {clip_id!r}: fp32 frames {tuple(frames.shape)} are not [n, 3, H, W] at the size of the first mask {hw}')
        if self._net_hw is not None and hw != self._net_hw:
            raise ValueError(f'RaggedGroupSlot: clip {clip_id!r} has network size {hw}, the slot runs {self._net_hw}: all clips of a '
                             'slot share one network size (bucket the clip list by size, one slot per size)')
        if c.host_u8:
            src = (int(frames.shape[1]), int(frames.shape[2]))
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f'RaggedGroupSlot: clip {clip_id!r}: uint8 frames must be [n, Hs, Ws, 3]')
            if self._src_hw is not None and src != self._src_hw:
                raise ValueError(f'RaggedGroupSlot: clip {clip_id!r} has uint8 frames of {src}, the slot stages {self._src_hw}: all '
                                 'clips of a slot share one frame size')
            self.feed.check_pinned(frames)
            if new_objects:
                raise ValueError('new_objects: frames must be fp32 device tensors at the network size')
            self._src_hw = src
        self._net_hw = hw
        if isinstance(new_objects, tuple):
            new_objects = {new_objects[0]: new_objects[1]}
        c.new_objects = {int(k): v for k, v in (new_objects or {}).items()}
        c.mask = first_mask
        c.gap = clip_gap(c.n) if gap is None else int(gap)
        c.labels = torch.zeros(c.n, self.out_hw[0], self.out_hw[1], dtype=torch.uint8, device=self.device)
        c.ready = None
        if self.device.type == 'cuda':             # the stack is zeroed on the caller's stream and written on the engine's
            c.ready = torch.cuda.Event()
            c.ready.record(torch.cuda.current_stream(self.device))
        (self._queue if c.n > 1 else self._trivial).append(c)

    @property
    def done(self) -> bool:
        """Queue empty and no live row."""
        return not self._queue and not self._trivial and not self._plan and not any(r.live for r in self._rows)

    def run(self, clips):
        """submit / step / yield until the iterable of (clip_id, frames, first_mask[, new_objects[, gap]]) and the rows are drained;
        the queue is kept two clips per row ahead."""
        it, dry = iter(clips), False
        while True:
            while not dry and len(self._queue) < 2 * self.clips:
                try:
                    self.submit(*next(it))
                except StopIteration:
                    dry = True
            if dry and self.done:
                return
            yield from self.step()

    # ------------------------------------------------------------------ device buffers
    def _buffers(self):
        if self.cur_label is not None:
            return
        dev, (H, W) = self.device, self._net_hw
        self.cur_label = torch.zeros(self.B, self.out_hw[0], self.out_hw[1], dtype=torch.uint8, device=dev)   # fixed address (graph-captured)
        self.routes = ops.LabelRoutes(self.cur_label, dev)
        # it was zeroed on the current stream; the engine's streams use it from here on
        for st in (self.engine.stream, self.engine.enc_stream):
            st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.engine.stream):    # zeroed on the stream that uses them: rows no clip has started in are encoded too
            self._first = self.feed.rows('first', (self.B, 3, H, W), zero=True)     # row-start frames (uint8 sources), look-ahead 1 input
        if self.flip:                                  # the twins' reference frames and first masks
            self._twin_img = self.feed.rows('twin_img', (self.clips, 3, H, W))
            self._twin_mask = self.feed.rows('twin_mask', (self.clips, 1, H, W))

    def _release(self):
        """Let go of finished clips whose frames no queued launch reads any more (no host wait: the events are only queried)."""
        self._retired = [(evs, c) for evs, c in self._retired if not all(e.query() for e in evs)]

    # ------------------------------------------------------------------ a new clip per row
    def _start(self, assign):
        """assign [(row, clip)]: frame 0 of each clip through the engine's row-start path; rows that have never held a clip and get
        none now take a copy of the first clip's reference frame as their bank entry and idle (a row the memory read has never run
        on is not built on); they hold no clip, so the first clip that moves into one is no refill."""
        eng, P = self.engine, self.clips
        if not self._started:
            eng.restart_engine()
        self._buffers()
        H, W = self._net_hw
        spare = []
        if not self._started:
            taken = {p for p, _ in assign}
            spare = [p for p in range(P) if p not in taken]
        rows, imgs, masks, gaps = [], [], [], []
        with torch.cuda.stream(eng.stream):
            s = eng.stream.cuda_stream
            for j, (p, c) in enumerate(assign):
                if c.ready is not None:
                    eng.stream.wait_event(c.ready)
                if c.host_u8:
                    self._ingest_frame(p, c.frames, 0)
                    img = self._first[p]
                else:
                    img = c.frames[0]
                mask = c.mask.reshape(1, H, W).float().contiguous()
                mine = [p] + (spare if j == 0 else [])
                rows.append(mine); imgs.append(img); masks.append(mask); gaps.append(c.gap)
                if self.flip:                                   # the twin: frame and first mask at the network size, THEN mirrored
                    self.feed.mirror(img, self._twin_img[p], s)
                    self.feed.mirror(mask, self._twin_mask[p], s)
                    rows.append([P + q for q in mine]); imgs.append(self._twin_img[p]); masks.append(self._twin_mask[p]); gaps.append(c.gap)
                row = self._rows[p]
                row.clip, row.i, row.live = c, 1, True
        eng.start_clips(rows, imgs, masks, gaps)
        self.frames_encoded += len(rows)
        if spare:
            eng.finish_clips(spare + ([P + q for q in spare] if self.flip else []))
        self._started = True

    def _take(self, p: int) -> Optional[_RaggedClip]:
        """The next queued clip for row p (None: queue dry)."""
        if not self._queue:
            return None
        if self._rows[p].clip is not None:
            self.refills += 1
        return self._queue.pop(0)

    # ------------------------------------------------------------------ look-ahead encoder
    def _kick(self, buf: int, plan):
        """Encode look-ahead batch ``plan`` ({row: (clip, first frame, new)}) into buffer ``buf`` on the engine's side stream
        (FrameFeed.kick; a new clip's ready event is waited for there).  frames_encoded counts as GroupSlot does: every row of the
        group for each frame index of the batch that some row needs."""
        feed_plan = {p: (c.frames, i, c.ready if is_new else None) for p, (c, i, is_new) in plan.items()}
        self.frames_encoded += self.B * self.feed.kick(self.engine, buf, feed_plan)

    def _ingest_frame(self, p: int, frames: torch.Tensor, i: int):
        """uint8 sources: frame i of row p's clip into _first[p] on the engine's main stream"""
        stage = self.feed.stage(self.clips, *self._src_hw)
        self.feed.ingest([(frames, i, 1, stage[p:], self._first[p:])], self.engine.stream.cuda_stream)

    def _boundary(self):
        """Look-ahead batch boundary: the clips planned for this batch start in their rows (cold: the rows are filled from the queue
        and the batch is encoded now), then the NEXT batch is planned -- rows that run on get their next frames, rows that end
        inside this batch (or idle) get the next queued clips' frames 1..lookahead -- and kicked."""
        eng, la = self.engine, self.engine.lookahead
        self._e = 0
        plan = self._plan
        cold = not plan
        if cold:
            plan = {}
            for p in range(self.clips):
                c = None if self._rows[p].live else self._take(p)
                if c is not None:
                    plan[p] = (c, 1, True)
            if not plan:
                return
        new = [(p, c) for p, (c, _, is_new) in plan.items() if is_new]
        if new:
            self._start(new)
        self._k += 1
        if cold:
            self._kick(self._k % 2, plan)
        nxt = {}
        for p, row in enumerate(self._rows):
            if row.live and row.i + la < row.clip.n:
                nxt[p] = (row.clip, row.i + la, False)
            else:
                c = self._take(p)
                if c is not None:
                    nxt[p] = (c, 1, True)
        self._plan = nxt or None
        if nxt:
            self._kick((self._k + 1) % 2, nxt)

    # ------------------------------------------------------------------ one frame of every live row
    def step(self, feed=None) -> List[FinishedClip]:
        """Every live row advances one frame: propagate, route the labels, update the memories.  feed: {clip_id: uint8 [Ho, Wo] device
        labels that go into that clip's memory update INSTEAD of the prediction} (the delivered labels stay the prediction).
        -> the clips that ended with this step."""
        eng, B, P = self.engine, self.B, self.clips
        la = eng.lookahead
        out: List[FinishedClip] = []
        self._release()
        for c in self._trivial:
            out.append(FinishedClip(c.id, c.labels, None, [0], []))
        self._trivial = []
        live = [p for p, r in enumerate(self._rows) if r.live]
        if la > 1:
            if self._e == 0 or not live:
                self._boundary()
        else:
            new = []
            for p, r in enumerate(self._rows):
                if not r.live:
                    c = self._take(p)
                    if c is not None:
                        new.append((p, c))
            if new:
                self._start(new)
        live = [p for p, r in enumerate(self._rows) if r.live]
        if not live:
            return out
        s = eng.stream.cuda_stream
        H, W = self._net_hw
        if la > 1:
            eng.propagate_to_labels(self.cur_label, enc_slot=(self._k % 2) * la + self._e)
            self._e = (self._e + 1) % la
        else:
            nb = 3 * H * W * 4
            for p in live:
                r = self._rows[p]
                if r.clip.host_u8:
                    self._ingest_frame(p, r.clip.frames, r.i)
                else:
                    ops.copy_async(self._first[p], r.clip.frames[r.i], nb)(s)
            if self.flip:
                self.feed.mirror(self._first[:P], self._first[P:], s)
            self.frames_encoded += B
            eng.propagate_to_labels(self.cur_label, imgs=self._first)
        self.row_steps_live += len(live)
        self.row_steps_idle += P - len(live)
        # ---- one launch routes every row's labels
        routes, inject = [], []
        for p, r in enumerate(self._rows):
            if not r.live:
                routes.append((None, None, None, -1, _lib.ROUTE_IDLE))
                continue
            ov = r.clip.new_objects.get(r.i)
            fd = feed.get(r.clip.id) if feed else None
            if ov is not None:
                inject.append(p)
            twin = P + p if self.flip and (ov is not None or fd is not None) else -1      # else the pair kernel wrote the twin's row
            routes.append((r.clip.labels[r.i], ov, fd, twin, _lib.ROUTE_LIVE))
        if self.flip:
            routes += [(None, None, None, -1, _lib.ROUTE_SKIP if r.live else _lib.ROUTE_IDLE) for r in self._rows]
        self.routes.upload(routes, s)
        self.routes.op(s)
        eng.update_from_labels(self.cur_label, skip=inject + [P + p for p in inject] if self.flip else inject)
        for p in inject:                          # the frame is re-added as a reference frame for that row (evaluator.py:484-508)
            r = self._rows[p]
            eng.add_reference_frame_for(p, r.clip.frames[r.i], self.cur_label[p])
            if self.flip:
                self.feed.mirror(r.clip.frames[r.i], self._twin_img[p], s)
                eng.add_reference_frame_for(P + p, self._twin_img[p], self.cur_label[P + p])
        ended = []
        for p in live:
            r = self._rows[p]
            r.i += 1
            if r.i >= r.clip.n:
                ended.append(p)
        if ended:
            traces = eng.finish_clips(ended + ([P + p for p in ended] if self.flip else []))
            ev = torch.cuda.Event()
            ev.record(eng.stream)
            ee = torch.cuda.Event()
            ee.record(eng.enc_stream)
            for j, p in enumerate(ended):
                r = self._rows[p]
                r.live = False
                idx, drops = traces[j]
                out.append(FinishedClip(r.clip.id, r.clip.labels, ev, idx, drops, traces[len(ended) + j] if self.flip else None))
                self._retired.append(((ev, ee), r.clip))
        return out
