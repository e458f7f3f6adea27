"""Throughput engine: the B rows of a group advance in lockstep through ONE set of launch lists.

The rows need not run clips of equal length.  The device side never asked for it: banks of different sizes share a key table
(rows padded with key_count 0), appends go through a per-row destination table, and one row can be restarted from a reference
frame while the others carry on (add_reference_frame_for).  ``start_clips`` is the per-row counterpart of
add_reference_frames: a NEW clip moves into a row, with its own frame counter and gap (bank_schedule.BankSchedule.start_clips),
while the other rows keep going; ``finish_clips`` hands out an ended clip's bank traces and leaves the row idle (its bank cut to
one frozen entry: never appended to, never scored, never part of T) until the next clip moves in.
clip_runner.RaggedGroupSlot drives a clip list of any lengths through a group this way (continuous batching); equal length is a
precondition of clip_runner.GroupSlot only, which starts all rows together with one shared frame counter and gap.

``GroupEngine`` is the batched counterpart of AOTEngine/AOTInferEngine (aot_engine.py) for clips with <= 10 objects whose
label masks are fed back.  Per clip it keeps exactly the host state AOTEngine keeps -- bank slot order,
``long_memories_indexes``, the eviction policy's EMA scores and visit counts (networks/layers/transformer.py:338-411), the
frame of the last long-term update (aot_engine.py:338-343), all in one rmem_ocu_amd.bank_schedule.BankSchedule with
clips = B.  Rows started together (add_reference_frames) share the engine's frame counter and gap, as clips of one length do
(managers/evaluator.py:330-335); rows started one by one (start_clips) count their own frames.
All device work goes through rmem_ocu_amd.group_runtime.GroupRuntime: one launch per layer for the whole group.

Covered protocols (the reference's evaluator, managers/evaluator.py:385-523):
  * restricted banks (N = former + latter, eviction by the RMem policy) and UNBOUNDED banks (latter_mem_len = 9999,
    tools/eval.py:92): the bank then grows by one entry per gap up to the 32 rows of the kernel's key table;
  * a NEW OBJECT appearing mid-clip in some of the clips (evaluator.py:484-508): that clip's frame is re-added as a reference
    frame -- its bank restarts at one entry and its long-term update schedule restarts at that frame (aot_engine.py:318-323),
    so from then on the clips of a group hold banks of DIFFERENT lengths and append at different frames.  The launches are laid
    out for the longest bank; shorter ones are padded with empty key-table rows (include/rmem.h: key_count 0), and bank appends
    go through the per-clip destination table (negative = no append for this clip).
R50-DeAOTL models run through group_runtime_deaot.GroupRuntimeDeAOT (same protocols; the eviction policy's scores and visit
counts then move on EVERY long-term update, deaot_engine.py / transformer.py:880-892).
SwinB-AOTL models (cfg 5) run through the same GroupRuntime with encoder_batch.SwinBatchEncoder as the look-ahead encoder.
FLIP TESTING (managers/evaluator.py:342-355, 427-441) runs inside a group too: with ``flip_tta=True`` the B = 2P rows are P
clips (rows 0..P-1) and their horizontally mirrored twins (rows P..2P-1).  A twin is one more clip of the same length and
network size, so launch lists, graphs, look-ahead and the per-row bank schedule / eviction policy / ``long_memories_indexes``
are unchanged (the reference gives every augmentation its own engine); the one coupling, after the decoder, is
ops.logits_post_flip_pairs in place of ops.logits_post: the mean of the pair's softmaxes, arg-maxed, written to the clip's
label row and mirrored to the twin's, with no full-size fp32 map in between.  clip_runner.GroupSlot mirrors the twins' frames,
first masks, new-object overlays and fed labels.
MULTI-SCALE TESTING (TEST_MULTISCALE, with or without flip) needs one network size per scale, so one GroupEngine per scale, each
a plain or flip group with its own runtime, streams and graphs: ``propagate_to_logits`` stops after the decoder and
clip_runner.MultiScaleGroupSlot merges the engines' logits into ONE label buffer (ops.logits_post_ms_merge), from which every
engine then updates its memory (update_from_labels resizes to its own network size).
Clips with > 10 objects run on the per-clip engines, which are the drop-in API.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from ... import ops
from ...bank_schedule import BankSchedule, bank_slots
from ...group_runtime import GroupRuntime, runtime_for

F32 = torch.float32


class GroupEngine:
    def __init__(self, aot_model, clips: int, gpu_id: int = 0, long_term_mem_gap: int = 9999, lookahead: int = 4, streams=None,
                 flip_tta: bool = False):
        if flip_tta and (clips < 2 or clips % 2):
            raise ValueError(f'GroupEngine(flip_tta=True): clips is the row count 2P, a clip and its mirrored twin per pair (got {clips})')
        self.flip_tta = flip_tta
        self.cfg = aot_model.cfg
        self.AOT = aot_model
        self.B = clips
        self.policy_every_update = self.cfg.MODEL_VOS == 'deaot'      # DeAOTEngine.policy_every_update
        self.gpu_id = gpu_id
        self.device = torch.device('cuda', gpu_id)
        self.align_corners = self.cfg.MODEL_ALIGN_CORNERS
        self.max_obj_num = aot_model.max_obj_num
        self.long_term_mem_gap = long_term_mem_gap
        self.lookahead = lookahead
        # streams = (main, encoder) made by the caller: the runtime deals streams onto its (4) hardware queues in CREATION order, so a
        # caller with several engines decides which streams share a queue by the order it creates them in (bench.py)
        self.stream = streams[0] if streams else torch.cuda.Stream(self.device)
        # the look-ahead encoder of the NEXT batch of frames runs here, beside the propagation of the current batch (events order
        # the two: a batch is propagated after its encoder finished, a buffer is re-encoded after its last frame was decoded)
        self.enc_stream = streams[1] if streams else torch.cuda.Stream(self.device)
        self._enc_done = [torch.cuda.Event(), torch.cuda.Event()]
        self._enc_free = [None, None]
        self.use_graphs = True
        self.rt: Optional[GroupRuntime] = None
        self._side: Optional[GroupRuntime] = None
        self._start_mask: Optional[torch.Tensor] = None      # start_clips: the first mask of the clip being started
        self._graphs = ops.GraphCache()
        self.bank = BankSchedule(self, clips)
        self.restart_engine()

    # ------------------------------------------------------------------ state
    def restart_engine(self):
        self.frame_step = 0
        self.obj_nums = None
        self.bank.restart(self.rt)

    def long_memories_indexes(self, clip: int) -> List[int]:
        return self.bank.long_memories_indexes(clip)

    @property
    def drop_trace(self) -> List[List[int]]:
        return self.bank.drop_trace

    def _s(self) -> int:
        return self.stream.cuda_stream

    def _ensure_runtime(self, H: int, W: int):
        slots = bank_slots(self.bank.n_keep)
        if self.rt is None or (self.rt.H, self.rt.W) != (H, W) or self.rt.S != slots:
            self.rt = runtime_for(self.AOT, (H, W), slots, self.device, self.B, self.lookahead)
            self._start_mask = None
            self.label_in = torch.empty(self.B, H, W, dtype=F32, device=self.device)
            self._graphs = ops.GraphCache()
            self._side = None
        return self.rt

    def _run(self, key: str, prog: list, s: Optional[int] = None):
        self._graphs.run(key, prog, self._s() if s is None else s, self.use_graphs)

    # ------------------------------------------------------------------ reference frames (aot_engine.py:241-325, all clips at once)
    def add_reference_frames(self, imgs: torch.Tensor, masks: torch.Tensor, obj_nums: int):
        """imgs [B, 3, H, W] fp32, masks [B, 1, H, W] label maps at the network size (device)."""
        B = self.B
        H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
        rt = self._ensure_runtime(H, W)
        self.obj_nums = [self.max_obj_num]            # AOTInferEngine forces this (aot_engine.py:697)
        with torch.cuda.stream(self.stream):
            s = self._s()
            ops.copy_async(rt.enc_now.img_in, imgs.contiguous(), B * 3 * H * W * 4)(s)
            self.label_in.copy_(masks.reshape(B, H, W), non_blocking=True)
            rt.prepare_pos(s)
            self.bank.start_reference(rt)
            self._run('ref', rt.prog_encode() + rt.prog_id_emb(self.label_in, H, W) + rt.prog_project(None) + rt.prog_lstt(True, 1) +
                      rt.prog_decode(None))

    def add_reference_frame_for(self, clip: int, img: torch.Tensor, label_u8: torch.Tensor):
        """Mid-clip reference frame for ONE clip of the group (a new object's mask arrived, evaluator.py:484-508 ->
        aot_engine.py:675-702, 241-325): img fp32 [3, H, W] at the network size, label_u8 uint8 [Ho, Wo] (the merged label map;
        resized to the network size by nearest neighbour inside the one-hot kernel) at a FIXED address.  The frame runs through a
        one-clip runtime of the group's class in reference mode (the same launch lists with clips = 1); its K / V become the clip's
        only bank entry and its short-term memory, the clip's long-term schedule restarts here, ``long_memories_indexes`` keeps
        growing (the reference's quirk, 323), the eviction policy's state is reset (init_memory, transformer.py:438-443)."""
        with torch.cuda.stream(self.stream):
            src = self._side_reference(img, label_u8)
            # the clip's bank := this frame only (aot_engine.py:322), short-term memory := this frame's (transformer.py:675-678)
            new = self.bank.start_reference(self.rt, [clip], append_table=False)[clip]      # the entry is copied in, not appended by a launch
            self._adopt_side_entry(clip, new, src)

    def _side_reference(self, img: torch.Tensor, label: torch.Tensor) -> int:
        """One frame through the one-clip side runtime in reference mode on the engine's stream (img fp32 [3, H, W], label uint8 or
        fp32 [hs, ws] at a FIXED address) -> the side bank slot that holds its K / V; its short-term memory is side.short_K / V."""
        rt = self.rt
        if self._side is None:
            self._side = runtime_for(self.AOT, (rt.H, rt.W), 1, self.device, 1, 1)         # one bank slot, one clip, no look-ahead
        side, s = self._side, self._s()
        hs, ws = int(label.shape[-2]), int(label.shape[-1])
        ops.copy_async(side.enc_now.img_in, img.contiguous(), 3 * rt.H * rt.W * 4)(s)
        side.prepare_pos(s)
        src = BankSchedule.restart_banks(side, [0], s)[0]
        ops.run(side.prog_encode() + side.prog_id_emb(label, hs, ws) + side.prog_project(None) + side.prog_lstt(True, 1), s)
        return src

    def _adopt_side_entry(self, c: int, new: int, src: int):
        """Row c's bank slot ``new`` and short-term memory := the side runtime's reference frame (stream-ordered copies)."""
        rt, side, s, L = self.rt, self._side, self._s(), self.rt.L
        for i in range(rt.NL):
            nk, nv = L * rt.bank_kw * 2, L * rt.bank_vw * 2          # bytes of one bank entry's keys / values
            ops.copy_async(rt.bank_K[i][c * rt.S + new], side.bank_K[i][src], nk)(s)
            ops.copy_async(rt.bank_V[i][c * rt.S + new], side.bank_V[i][src], nv)(s)
            ops.copy_async(rt.short_K[i][c * L:(c + 1) * L], side.short_K[i], nk)(s)
            ops.copy_async(rt.short_V[i][c * L:(c + 1) * L], side.short_V[i], nv)(s)

    # ------------------------------------------------------------------ ragged groups: a new clip per row
    def start_clips(self, rows: List[List[int]], imgs: List[torch.Tensor], masks: List[torch.Tensor], gaps: List[int]):
        """Per-row counterpart of add_reference_frames: clip j starts in the rows ``rows[j]`` (one row; several when the same clip
        fills rows that would otherwise never have held a bank entry) while the other rows carry on.  imgs[j] fp32 [3, H, W] and
        masks[j] fp32 [H, W] label map, both at the network size; gaps[j] the clip's long_term_mem_gap.  With flip_tta the caller
        passes a clip for row p and its mirrored twin (frame and mask resized, THEN mirrored) for row P + p in the same call.  The
        frame runs through the one-clip side runtime (add_reference_frame_for's machinery); the rows' index lists, drop traces,
        policies and frame counters start over (BankSchedule.start_clips), which is what tells a new clip from a mid-clip
        reference frame."""
        H, W = int(imgs[0].shape[-2]), int(imgs[0].shape[-1])
        rt = self._ensure_runtime(H, W)
        self.obj_nums = [self.max_obj_num]            # AOTInferEngine forces this (aot_engine.py:697)
        if self._start_mask is None or tuple(self._start_mask.shape) != (H, W):
            # fixed address: the side launch list names it.  empty, not zeros: every byte is written on the engine's stream before
            # it is read there, and a fill enqueued on the caller's stream would not be ordered against that copy
            self._start_mask = torch.empty(H, W, dtype=F32, device=self.device)
        with torch.cuda.stream(self.stream):
            s = self._s()
            rt.prepare_pos(s)
            flat = [r for rs in rows for r in rs]
            first = self.bank.start_clips(rt, flat, [g for rs, g in zip(rows, gaps) for _ in rs])
            for rs, img, mask in zip(rows, imgs, masks):
                ops.copy_async(self._start_mask, mask.reshape(H, W).contiguous(), H * W * 4)(s)
                src = self._side_reference(img, self._start_mask)
                for r in rs:
                    self._adopt_side_entry(r, first[r], src)

    def finish_clips(self, rows: List[int]):
        """The clips of ``rows`` have ended -> [(long_memories_indexes, drop_trace)]; the rows idle until start_clips."""
        with torch.cuda.stream(self.stream):
            return self.bank.finish_clips(self.rt, rows)

    # ------------------------------------------------------------------ look-ahead encoder
    def encode_inputs(self, buf: int = 0) -> torch.Tensor:
        """fp32 [lookahead * B, 3, H, W] of look-ahead buffer ``buf``: frame e of clip c goes to row e * B + c.  Fill it on
        ``enc_stream`` (the previous encoder pass over this buffer reads it there)."""
        return self.rt.enc_bufs[buf].img_in

    def encode_ahead(self, buf: int = 0):
        """Encode the frames in encode_inputs(buf) on the side stream; propagate_to_labels(enc_slot = buf * lookahead + e)
        waits for it."""
        es = self.enc_stream
        if self._enc_free[buf] is not None:
            es.wait_event(self._enc_free[buf])          # the buffer's previous frames have been projected / decoded
        with torch.cuda.stream(es):
            self._run(f'encB{buf}', self.rt.enc_bufs[buf].prog(), es.cuda_stream)
            self._enc_done[buf].record(es)

    # ------------------------------------------------------------------ propagate (aot_engine.py:398-465 + evaluator.py:430-441)
    def propagate_to_labels(self, labels_u8: torch.Tensor, enc_slot: Optional[int] = None, imgs: Optional[torch.Tensor] = None):
        """labels_u8: uint8 [B, Ho, Wo] device buffer at a fixed address.  Either enc_slot (frame encoded by encode_ahead) or
        imgs [B, 3, H, W] (encoded now).  flip_tta: rows p and B/2 + p are merged; row p gets the label, row B/2 + p its mirror."""
        self.frame_step += 1
        self.bank.advance()                           # rows started by start_clips count their own frames
        rt, B = self.rt, self.B
        T, wm = self.bank.begin_propagation(rt)
        Ho, Wo = int(labels_u8.shape[-2]), int(labels_u8.shape[-1])
        with torch.cuda.stream(self.stream):
            pk = f'post_{labels_u8.data_ptr()}_{Ho}_{Wo}'
            if pk not in rt._prog:
                if self.flip_tta:
                    post = ops.logits_post_flip_pairs(rt.logits, nc=rt.nc, keep=self.obj_nums[0], Hi=rt.H4, Wi=rt.W4, Ho=Ho, Wo=Wo,
                                                      align_corners=self.align_corners, label_u8=labels_u8, rows=B)
                else:
                    post = ops.logits_post(rt.logits, ldl=16, nc=rt.nc, keep=self.obj_nums[0], Hi=rt.H4, Wi=rt.W4, Ho=Ho, Wo=Wo,
                                           align_corners=self.align_corners, label_u8=labels_u8, images=B)
                rt._prog[pk] = [post]
            self._propagate(T, wm, rt._prog[pk], f'_{labels_u8.data_ptr()}', enc_slot, imgs)

    def _propagate(self, T: int, wm: bool, post: list, tag: str, enc_slot: Optional[int], imgs: Optional[torch.Tensor]):
        """(encode,) project, LSTT, decode, then ``post`` on the engine's stream (already current); graph key prop<T><wm>e<slot><tag>"""
        rt, B = self.rt, self.B
        if enc_slot is None:
            ops.copy_async(rt.enc_now.img_in, imgs.contiguous(), B * 3 * rt.H * rt.W * 4)(self._s())
            prog = rt.prog_encode() + rt.prog_project(None) + rt.prog_lstt(False, T, wm) + rt.prog_decode(None) + post
        else:
            buf = enc_slot // rt.lookahead
            self.stream.wait_event(self._enc_done[buf])
            prog = rt.prog_project(enc_slot) + rt.prog_lstt(False, T, wm) + rt.prog_decode(enc_slot) + post
        self._run(f'prop{T}{int(wm)}e{enc_slot}{tag}', prog)
        if enc_slot is not None:
            ev = self._enc_free[buf] or torch.cuda.Event()
            ev.record(self.stream)
            self._enc_free[buf] = ev

    def propagate_to_logits(self, enc_slot: Optional[int] = None, imgs: Optional[torch.Tensor] = None) -> torch.cuda.Event:
        """propagate_to_labels without the post-processing launch: the group's 1/4-resolution logits stay in ``rt.logits`` (fp32
        [B, H4*W4, 16]) for a merge across engines (clip_runner.MultiScaleGroupSlot, ops.logits_post_ms_merge).  Returns an event
        recorded on the engine's stream behind them; ``rt.logits`` is rewritten by this engine's next propagation only.  Graph keys
        of its own (prop..._logits): the launch lists of propagate_to_labels are not touched."""
        self.frame_step += 1
        self.bank.advance()
        T, wm = self.bank.begin_propagation(self.rt)
        with torch.cuda.stream(self.stream):
            self._propagate(T, wm, [], '_logits', enc_slot, imgs)
            if getattr(self, '_logits_ready', None) is None:
                self._logits_ready = torch.cuda.Event()
            self._logits_ready.record(self.stream)
        return self._logits_ready

    # ------------------------------------------------------------------ memory update (aot_engine.py:327-369)
    def update_from_labels(self, labels_u8: torch.Tensor, skip: Iterable[int] = ()):
        """labels_u8: uint8 [B, Ho, Wo] argmax labels at the output size (nearest-resized to the network size on the device).
        skip: clips whose memory is re-initialised right after by add_reference_frame_for (no bank append for them)."""
        rt = self.rt
        hs, ws = int(labels_u8.shape[-2]), int(labels_u8.shape[-1])
        with torch.cuda.stream(self.stream):
            slots = self.bank.take_append_slots(rt, skip)
            appends = max(slots) >= 0
            self._run(f'upd{int(appends)}_{labels_u8.data_ptr()}', rt.prog_id_emb(labels_u8, hs, ws) + rt.prog_update(appends))
            self.bank.commit_update(rt, slots, self.obj_nums[0])

    def synchronize(self):
        self.stream.synchronize()
        self.enc_stream.synchronize()
