"""Per-clip inference engines with the reference's method surface.

``AOTEngine`` mirrors networks/engines/aot_engine.py:18-568 (inference half) and
``AOTInferEngine`` mirrors 571-725: same method names, arguments, attributes
(``long_term_mem_gap, input_size_2d, enc_size_2d, enc_hw, long_memories_indexes``) and
error behaviour; the math runs as the HIP launch lists of a one-clip
rmem_ocu_amd.group_runtime.GroupRuntime (the class GroupEngine runs with clips = B).  What
stays on the host is exactly what the reference keeps in Python: the frame counter, the
"append every ``gap`` frames" rule (338-343), and the restricted-memory eviction policy
(layers/transformer.py:324-436): both live in rmem_ocu_amd.bank_schedule.BankSchedule, which the engine holds with clips = 1.

Differences by design: clip state is engine-owned (the reference stores it in
the shared model); bs = 1 per engine (the reference asserts it in eval,
layers/transformer.py:641); the attention-weight top-32 D2H of every layer
(transformer.py:644-648) is not produced (only dead code consumed it).
"""
from __future__ import annotations

import contextlib
from typing import List, Optional

import numpy as np
import torch

from ... import ops
from ...bank_schedule import BankSchedule, MemoryPolicy, bank_slots       # noqa: F401  (MemoryPolicy: part of this module's surface)
from ...group_runtime import GroupRuntime, runtime_for

F32 = torch.float32


class AOTEngine:
    policy_every_update = False      # DeAOT: scores / visit counts move on every long-term update (deaot_engine.py)

    def __init__(self, aot_model, gpu_id=0, long_term_mem_gap=9999, short_term_mem_skip=1):
        self.cfg = aot_model.cfg
        self.align_corners = aot_model.cfg.MODEL_ALIGN_CORNERS
        self.AOT = aot_model
        self.max_obj_num = aot_model.max_obj_num
        self.gpu_id = gpu_id
        self.long_term_mem_gap = long_term_mem_gap
        self.short_term_mem_skip = short_term_mem_skip
        if short_term_mem_skip != 1:
            raise NotImplementedError('short_term_mem_skip != 1 is not used by the reference evaluator')
        self.device = torch.device('cuda', gpu_id)
        # every engine enqueues on its own HIP stream (clips overlap on the GPU; the null stream cannot be
        # captured into a hipGraph); sync_caller orders it after/before the caller's current stream like
        # the reference's default-stream semantics
        self.stream = torch.cuda.Stream(self.device)
        self.sync_caller = True
        self.rt: Optional[GroupRuntime] = None
        self.use_graphs = False
        self._graphs = ops.GraphCache()
        self.bank = BankSchedule(self, 1)
        self.restart_engine()

    # ------------------------------------------------------------------ state
    def restart_engine(self, batch_size=1, enable_id_shuffle=False):
        if batch_size != 1 or enable_id_shuffle:
            raise NotImplementedError('inference engine: batch_size 1, no id shuffle (layers/transformer.py:641)')
        self.batch_size = 1
        self.frame_step = 0
        self.obj_nums = None
        self.input_size_2d = None
        self.enc_size_2d = None
        self.enc_hw = None
        self.pred_id_logits = None
        self.bank.restart(self.rt)

    def eval(self):
        return self

    @property
    def long_memories_indexes(self) -> List[int]:
        """Frame indexes of the bank entries (aot_engine.py:323, 351); resolves a deferred eviction first."""
        return self.bank.long_memories_indexes(0)

    @property
    def drop_trace(self) -> List[int]:
        return self.bank.drop_trace[0]

    @property
    def last_mem_step(self) -> int:
        return self.bank.last_mem_step[0]

    def update_size(self, input_size, enc_size):
        self.input_size_2d = tuple(int(v) for v in input_size)
        self.enc_size_2d = tuple(int(v) for v in enc_size)
        self.enc_hw = self.enc_size_2d[0] * self.enc_size_2d[1]

    def _stream(self) -> int:
        return self.stream.cuda_stream

    @contextlib.contextmanager
    def _scope(self):
        cur = torch.cuda.current_stream(self.device)
        if self.sync_caller:
            self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield cur
        if self.sync_caller:
            cur.wait_stream(self.stream)

    def _ensure_runtime(self, img):
        H, W = int(img.shape[-2]), int(img.shape[-1])
        if self.rt is None or (self.rt.H, self.rt.W) != (H, W):
            # one clip, no look-ahead encoder until encode_ahead asks for one
            self.rt = runtime_for(self.AOT, (H, W), bank_slots(self.bank.n_keep), self.device, 1, lookahead=1)
            self.img_in = self.rt.enc_now.img_in[0]         # fixed address: what the encoder's pointer table names
            self.label_in = torch.empty(H, W, dtype=F32, device=self.device)
            self._graphs = ops.GraphCache()
        return self.rt

    def _run(self, key: str, prog: list):
        """Enqueue a launch list on the engine's stream: directly, or (use_graphs) as ONE hipGraph per key."""
        self._graphs.run(key, prog, self._stream(), self.use_graphs)

    def _set_label(self, mask):
        m = mask.reshape(mask.shape[-2], mask.shape[-1])
        if tuple(m.shape) != (self.rt.H, self.rt.W):
            raise ValueError(f'mask must be at the network size {(self.rt.H, self.rt.W)}, got {tuple(m.shape)}')
        self._copy_in(self.label_in, m)

    def _copy_in(self, dst, src):
        """Frame / label into the engine's fixed input buffer on the engine's stream: a plain memcpy node through the C ABI when
        the caller's tensor already has the buffer's type and layout (the evaluator's do), torch's converting copy otherwise."""
        if src.is_cuda and src.dtype == dst.dtype and src.is_contiguous():
            ops.copy_async(dst, src, dst.numel() * dst.element_size())(self._stream())
        else:
            dst.copy_(src, non_blocking=True)

    # ------------------------------------------------------------------ reference frame
    def add_reference_frame(self, img=None, mask=None, frame_step=-1, obj_nums=None, img_embs=None):
        if self.obj_nums is None and obj_nums is None:
            print('No objects for reference frame!')
            exit()
        elif obj_nums is not None:
            self.obj_nums = obj_nums
        if frame_step == -1:
            frame_step = self.frame_step
        if img is None:
            print('No image for reference frame!')
            exit()
        if mask is None:
            print('No mask for reference frame!')
            exit()
        rt = self._ensure_runtime(img)
        if self.input_size_2d is None:
            self.update_size(img.shape[2:], (rt.H16, rt.W16))
        with self._scope():
            self._copy_in(self.img_in, img.reshape(3, rt.H, rt.W))
            self._set_label(mask)
            # (re)initialise the bank to this frame only (aot_engine.py:322; quirk: long_memories_indexes keeps growing, 323)
            rt.prepare_pos(self._stream())
            self.bank.start_reference(rt, mem_step=frame_step)
            self._run('ref', rt.prog_encode() + rt.prog_id_emb(self.label_in, rt.H, rt.W) + rt.prog_project(None) +
                      rt.prog_lstt(True, 1) + rt.prog_decode(None))
            self.pred_id_logits = rt.logits

    # ------------------------------------------------------------------ propagate
    def match_propogate_one_frame(self, img=None, img_embs=None, mask=None, output_size=None):
        self.frame_step += 1
        if img is None:
            raise ValueError('match_propogate_one_frame needs the frame (offline encoding is a training-only path)')
        rt = self.rt
        T, wm = self.bank.begin_propagation(rt)
        with self._scope() as cur:
            self._copy_in(self.img_in, img.reshape(3, rt.H, rt.W))
            self._run(f'prop{T}{int(wm)}', rt.prog_encode() + rt.prog_project(None) + rt.prog_lstt(False, T, wm) + rt.prog_decode(None))
            self.pred_id_logits = rt.logits
            out = self._logits_out(output_size)
            out.record_stream(cur)
        return out

    def encode_ahead(self, imgs, frames: int = 4):
        """Run the ResNet-50 encoder for the next ``imgs.shape[0] <= frames`` frames of the clip as one launch per layer
        (frames do not depend on each other before the LSTT; the reference's loader has them ready,
        dataloaders/eval_datasets.py:57-64).  propagate_to_label(..., enc_slot=e) then consumes frame e."""
        rt, be = self.rt, self._ahead(frames)
        with self._scope():
            if imgs is not None:                      # None: the caller already put the frames into encode_inputs(frames)
                n = int(imgs.shape[0])
                if n > frames:
                    raise ValueError(f'encode_ahead: {n} frames for a look-ahead of {frames}')
                ops.copy_async(be.img_in, imgs, n * 3 * rt.H * rt.W * 4)(self._stream())
            self._run(f'encB{frames}', be.prog())

    def encode_inputs(self, frames: int = 4):
        """fp32 [frames, 3, H, W] input buffer of encode_ahead (e.g. the target of rmem_ingest_rgb8, so decoded uint8 frames
        go host -> device -> resize + normalise -> encoder without an extra copy)."""
        return self._ahead(frames).img_in

    def _ahead(self, frames: int):
        """The engine's one look-ahead encoder of ``frames`` frames (look-ahead buffer 0 of the runtime), built on first use."""
        rt = self.rt
        if not rt.enc_bufs or rt.lookahead != frames:
            rt.build_lookahead(1, frames)
            # captured lists that run or read the previous look-ahead buffers
            self._graphs.drop(('encB', 'propl'))
        return rt.enc_bufs[0]

    def propagate_to_label(self, img, label_u8, enc_slot=None):
        """Fused fast path of one frame: propagate, then argmax labels (uint8 [Ho, Wo], caller's device
        buffer at a fixed address) straight from the 1/4-resolution logits -- the evaluator's
        softmax -> argmax (managers/evaluator.py:430-441) without materialising [11, Ho, Wo] logits.
        enc_slot: the frame was encoded by encode_ahead (slot index); img is then unused."""
        self.frame_step += 1
        rt = self.rt
        T, wm = self.bank.begin_propagation(rt)
        Ho, Wo = int(label_u8.shape[-2]), int(label_u8.shape[-1])
        with self._scope():
            pk = f'post_{label_u8.data_ptr()}_{Ho}_{Wo}'
            if pk not in rt._prog:
                rt._prog[pk] = [ops.logits_post(rt.logits, ldl=16, nc=rt.nc, keep=self._keep(), Hi=rt.H4, Wi=rt.W4, Ho=Ho, Wo=Wo,
                                                align_corners=self.align_corners, label_u8=label_u8)]
            if enc_slot is None:
                ops.copy_async(self.img_in, img, 3 * rt.H * rt.W * 4)(self._stream())
                key = f'propl{T}{int(wm)}_{label_u8.data_ptr()}_{Ho}_{Wo}'
                self._run(key, rt.prog_encode() + rt.prog_project(None) + rt.prog_lstt(False, T, wm) + rt.prog_decode(None) + rt._prog[pk])
            else:
                key = f'propl{T}{int(wm)}e{enc_slot}_{label_u8.data_ptr()}_{Ho}_{Wo}'
                self._run(key, rt.prog_project(enc_slot) + rt.prog_lstt(False, T, wm) + rt.prog_decode(enc_slot) + rt._prog[pk])
            self.pred_id_logits = rt.logits

    def _keep(self) -> int:
        """Highest object id in use: logits and eviction scores mask the ids above it (aot_engine.py:450-453)."""
        return self.obj_nums[0] if self.obj_nums else self.max_obj_num

    def decode_current_logits(self, output_size=None):
        """Logits with unused ids masked (aot_engine.py:450-453), resized to output_size (457-463)."""
        with self._scope() as cur:
            out = self._logits_out(output_size)
            out.record_stream(cur)
        return out

    def _logits_out(self, output_size=None):
        rt = self.rt
        Ho, Wo = (rt.H4, rt.W4) if output_size is None else (int(output_size[0]), int(output_size[1]))
        out = torch.empty(1, rt.nc, Ho, Wo, dtype=F32, device=self.device)
        ops.run(ops.logits_post(rt.logits, ldl=16, nc=rt.nc, keep=self._keep(), Hi=rt.H4, Wi=rt.W4, Ho=Ho, Wo=Wo,
                                align_corners=self.align_corners, out=out), self._stream())
        return out

    def predict_current_mask(self, output_size=None, return_prob=False):
        """aot_engine.py:467-483."""
        if output_size is None:
            output_size = self.input_size_2d
        logits = self.decode_current_logits(output_size)
        pred_mask = torch.argmax(logits, dim=1)
        return (pred_mask, torch.softmax(logits, dim=1)) if return_prob else pred_mask

    # ------------------------------------------------------------------ memory update
    def update_short_term_memory(self, curr_mask, curr_id_emb=None, step=0):
        if curr_id_emb is not None:
            raise NotImplementedError('update_short_term_memory takes the label mask')
        rt = self.rt
        if curr_mask.dim() == 4 and curr_mask.shape[1] != 1:
            raise NotImplementedError('probability masks (>10 objects soft aggregation) are not built yet')
        with self._scope():
            self._set_label(curr_mask)
            self._finish_update('lab', rt.prog_id_emb(self.label_in, rt.H, rt.W))
        if self.sync_caller:
            self.bank.resolve()          # drop-in semantics: long_memories_indexes is exact when the call returns

    def update_memory_from_label_u8(self, label_u8: torch.Tensor):
        """Fast path: argmax labels at the OUTPUT size (uint8 [Ho, Wo], device); the nearest resize to the
        network size (evaluator.py:518-522) happens inside the one-hot kernel."""
        rt = self.rt
        hs, ws = int(label_u8.shape[-2]), int(label_u8.shape[-1])
        with self._scope():
            self._finish_update(f'u8_{label_u8.data_ptr()}', rt.prog_id_emb(label_u8, hs, ws))

    def _finish_update(self, id_key: str, id_prog: list):
        """Memory update of the frame just propagated (aot_engine.py:327-369).  The launch list (identity embedding +
        short-term update [+ bank append]) is one graph; whether the bank is appended to, and the eviction that may follow
        (decided lazily, right before the bank is used again, so the host never waits here), is the schedule's."""
        rt = self.rt
        slots = self.bank.take_append_slots(rt)
        update_long = slots[0] >= 0
        self._run(f'upd{int(update_long)}_{id_key}', id_prog + rt.prog_update(update_long))
        self.bank.commit_update(rt, slots, self._keep())


class AOTInferEngine:
    ENGINE = AOTEngine

    def __init__(self, aot_model, gpu_id=0, long_term_mem_gap=9999, short_term_mem_skip=1, max_aot_obj_num=None):
        self.cfg = aot_model.cfg
        self.AOT = aot_model
        if max_aot_obj_num is None or max_aot_obj_num > aot_model.max_obj_num:
            self.max_aot_obj_num = aot_model.max_obj_num
        else:
            self.max_aot_obj_num = max_aot_obj_num
        self.gpu_id = gpu_id
        self.long_term_mem_gap = long_term_mem_gap
        self.short_term_mem_skip = short_term_mem_skip
        self.use_graphs = False
        self.aot_engines: List[AOTEngine] = []
        self._pool: List[AOTEngine] = []
        self.restart_engine()

    def eval(self):
        return self

    def restart_engine(self):
        for engine in self.aot_engines:
            engine.restart_engine()
        self._pool = self.aot_engines + [e for e in self._pool if e not in self.aot_engines]
        self.aot_engines = []
        self.obj_nums = None

    def separate_mask(self, mask):
        """aot_engine.py:604-628 (label-map branch): engine e keeps ids e*10+1 .. (e+1)*10, renumbered from 1 (rmem_split_label)."""
        if mask is None:
            return [None] * len(self.aot_engines)
        if len(self.aot_engines) == 1:
            return [mask]
        if mask.dim() == 3 or mask.shape[0] == 1:
            import ctypes as C
            from ... import _lib
            m = mask.to(F32).contiguous()
            s = torch.cuda.current_stream(m.device).cuda_stream
            out = []
            for idx in range(len(self.aot_engines)):
                o = torch.empty_like(m)
                _lib.check(_lib.lib().rmem_split_label(m.data_ptr(), idx * self.max_aot_obj_num + 1, (idx + 1) * self.max_aot_obj_num,
                                                       o.data_ptr(), m.numel(), C.c_void_p(s)), 'rmem_split_label')
                out.append(o)
            return out
        raise NotImplementedError('probability masks for >10 objects')

    def soft_logit_aggregation(self, all_logits):
        """aot_engine.py:650-673 as one HIP launch (rmem_soft_logit_aggregate)."""
        if len(all_logits) == 1:
            return all_logits[0]
        import ctypes as C
        from ... import _lib
        n = len(all_logits)
        lg = [t.contiguous() for t in all_logits]
        _, nc, H, W = lg[0].shape
        out = torch.empty(1, 1 + n * self.max_aot_obj_num, H, W, dtype=F32, device=lg[0].device)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in lg])
        _lib.check(_lib.lib().rmem_soft_logit_aggregate(ptrs, n, nc, self.max_aot_obj_num, H, W, out.data_ptr(),
                                                        C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)),
                   'rmem_soft_logit_aggregate')
        return out

    def add_reference_frame(self, img, mask, obj_nums, frame_step=-1):
        if isinstance(obj_nums, list):
            obj_nums = obj_nums[0]
        aot_num = max(np.ceil(obj_nums / self.max_aot_obj_num), 1)
        while aot_num > len(self.aot_engines):
            if self._pool:
                eng = self._pool.pop(0)           # reuse device buffers of an earlier clip
                eng.long_term_mem_gap = self.long_term_mem_gap
            else:
                eng = self.ENGINE(self.AOT, self.gpu_id, self.long_term_mem_gap, self.short_term_mem_skip)
            eng.use_graphs = self.use_graphs
            eng.sync_caller = not getattr(self, '_async', False)
            self.aot_engines.append(eng)
        for eng, m in zip(self.aot_engines, self.separate_mask(mask)):
            eng.add_reference_frame(img, m, obj_nums=[self.max_aot_obj_num], frame_step=frame_step)
        self.update_size()

    def match_propogate_one_frame(self, img=None, mask=None, output_size=None):
        all_logits = [e.match_propogate_one_frame(img, mask=mask, output_size=output_size) for e in self.aot_engines]
        return self.soft_logit_aggregation(all_logits)

    def update_memory(self, curr_mask):
        for eng, m in zip(self.aot_engines, self.separate_mask(curr_mask)):
            eng.update_short_term_memory(m)

    # -- fused fast path (single engine, <= 10 objects): labels in, labels out, everything on the engine's stream
    def propagate_to_label(self, img, label_u8, enc_slot=None):
        if len(self.aot_engines) != 1:
            raise NotImplementedError('the fused label path covers clips with <= 10 objects')
        self.aot_engines[0].propagate_to_label(img, label_u8, enc_slot)

    def encode_ahead(self, imgs, frames: int = 4):
        if len(self.aot_engines) != 1:
            raise NotImplementedError('encoder look-ahead covers clips with <= 10 objects')
        self.aot_engines[0].encode_ahead(imgs, frames)

    def encode_inputs(self, frames: int = 4):
        return self.aot_engines[0].encode_inputs(frames)

    def update_memory_from_label_u8(self, label_u8):
        self.aot_engines[0].update_memory_from_label_u8(label_u8)

    def set_async(self, use_graphs=True):
        """Detach the engines from the caller's stream (each clip runs on its own stream) and replay frames as hipGraphs."""
        self.use_graphs = use_graphs
        for e in self.aot_engines + self._pool:
            e.use_graphs = use_graphs
            e.sync_caller = False
        self._async = True

    def synchronize(self):
        for e in self.aot_engines:
            e.stream.synchronize()

    def update_size(self):
        self.input_size_2d = self.aot_engines[0].input_size_2d
        self.enc_size_2d = self.aot_engines[0].enc_size_2d
        self.enc_hw = self.aot_engines[0].enc_hw

    @property
    def long_memories_indexes(self):
        return self.aot_engines[0].long_memories_indexes
