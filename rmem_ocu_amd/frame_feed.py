"""How the frames of clips reach the encoder's fp32 input rows: the one place (outside ops.py) that stages and ingests uint8
sources, mirrors flip twins and fills a look-ahead batch.  A slot of clip_runner owns one FrameFeed and keeps the bookkeeping
(rows, labels, counters, lifetimes); the feed owns the buffers that frames pass through.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from . import ops
from .jpeg import JpegClip


def lookahead_rows(plan: Dict[int, tuple], B: int, P: int, lookahead: int, flip: bool) -> List[tuple]:
    """The encoder's pointer table for a look-ahead batch of fp32 sources, as names: entry k * B + r for frame index k of row r.
    plan {row: (source, first frame index, ...)}, rows 0..P-1; B = 2P with flip (rows P.. are the mirrored twins), else B = P.
      ('frame', r, min(i + k, n - 1))   frame of row r's source (beyond the clip's end its last frame again: encoded, never used)
      ('twin', r, min(k, m - 1))        twin staging [r, .] of the m = min(lookahead, n - i) frames mirrored for this batch
      ('idle',)                         a row without a plan, and its twin: the feed's own idle frame, never a finished clip's"""
    table = [('idle',)] * (lookahead * B)
    for r, v in plan.items():
        i, last = v[1], v[0].shape[0] - 1
        for k in range(lookahead):
            table[k * B + r] = ('frame', r, min(i + k, last))
            if flip:
                table[k * B + P + r] = ('twin', r, min(k, last - i))        # = min(k, m - 1), as k < lookahead
    return table


class FrameFeed:
    """Frames of B rows (P clips; with flip B = 2P and rows P.. are the clips' mirrored twins) on their way into an engine.

    Buffers are allocated on first use and again when their size changes.  STREAMS: stage() rows belong to the slot's main stream;
    kick() has its own uint8 staging and per-look-ahead-buffer twin staging, written and read on the encoder stream only, so the
    main stream's row starts and steps run beside a kick without sharing a row with it."""

    def __init__(self, device, B: int = 1, P: int = 1, lookahead: int = 1, flip: bool = False):
        self.device = torch.device(device)
        self.B, self.P, self.lookahead, self.flip = B, P, max(lookahead, 1), flip
        self._bufs: Dict[str, torch.Tensor] = {}
        self._zeroed_rt = None                 # the runtime whose look-ahead encoder inputs have been zeroed

    def _buf(self, name: str, shape: Tuple[int, ...], dtype, zero: bool = False) -> torch.Tensor:
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._bufs[name] = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.device)
        return t

    def stage(self, n: int, hs: int, ws: int) -> torch.Tensor:
        """uint8 [n, hs, ws, 3] staging rows of the main stream."""
        return self._buf('stage', (n, hs, ws, 3), torch.uint8)

    def rows(self, name: str, shape, zero: bool = False) -> torch.Tensor:
        """A named fp32 buffer ('first': ingested row-start / per-frame inputs; 'twin_img', 'twin_mask', 'twin_ref': mirrored
        reference frames and first masks).  zero: filled on the CURRENT stream when (re)allocated -- call it under the stream that
        uses the buffer."""
        return self._buf(name, tuple(shape), torch.float32, zero)

    def check_pinned(self, source):
        if self.device.type == 'cuda' and not source.is_pinned():
            raise ValueError('uint8 host frames must be in pinned memory')

    def ingest(self, jobs, stream: int):
        """jobs [(source, i, m, stage, dst)]: frames i .. i+m-1 of a uint8 source into the staging rows stage[0:m] -- an H2D copy of
        pinned uint8 frames [n, hs, ws, 3], or for a JpegClip the copy of their compressed bytes and the GPU decode straight into
        those rows -- and from there, resized and normalised (rmem_ingest_rgb8), into the fp32 [3, H, W] rows dst[0:m]; all on
        ``stream``, every job's load ahead of the first ingest (copies and kernels that alternate on a stream cost host time)."""
        todo = []
        for source, i, m, stage, dst in jobs:
            hs, ws = int(stage.shape[1]), int(stage.shape[2])
            if isinstance(source, JpegClip):
                source.decode_into(list(stage[:m]), i, m, stream)
            else:
                ops.copy_async(stage, source[i:i + m], m * hs * ws * 3)(stream)
            H, W = int(dst[0].shape[-2]), int(dst[0].shape[-1])
            todo += [ops.ingest_rgb8(stage[k], Hs=hs, Ws=ws, Hd=H, Wd=W, out_chw=dst[k]) for k in range(m)]
        ops.run(todo, stream)

    def mirror(self, src: torch.Tensor, dst: torch.Tensor, stream: int):
        """dst := src mirrored along W (fp32, equal shapes: rmem_resize_nearest_flip_f32 at equal size): how every twin is made."""
        ops.run(ops.resize_nearest_flip(src, dst, flip=True), stream)

    def kick(self, engine, buf: int, plan: Dict[int, tuple]) -> int:
        """Encode a look-ahead batch into buffer ``buf`` on the engine's side stream.  plan {row: (source, first frame index, ready
        event or None)}: frames first .. first + lookahead - 1 of each planned row; ready: waited for on the encoder stream (the
        first time that stream touches the clip).  uint8 sources are staged and ingested into encode_inputs(buf) rows k * B + row
        (rows without a plan keep what they hold: zeros, or an ended clip's frames); fp32 sources are read where they are through
        the encoder's pointer table (lookahead_rows).  Twins are mirrored here, on the encoder stream, ahead of the encoder launch
        that _enc_done / _enc_free order against the propagation.  -> the largest min(lookahead, n - first) over the plan: the
        frame indexes of the batch that some row needs."""
        B, P, la = self.B, self.P, self.lookahead
        es = engine.enc_stream.cuda_stream
        enc = engine.rt.enc_bufs[buf]
        need = {}
        for r, (src, i, ready) in plan.items():
            need[r] = min(la, src.shape[0] - i)
            if ready is not None:
                engine.enc_stream.wait_event(ready)
        if src.dtype == torch.uint8:                            # the clips of a slot share source kind and sizes
            enc.point_at_img_in(es)
            dst = engine.encode_inputs(buf)
            if self._zeroed_rt is not engine.rt:                # rows that are never ingested into must still hold numbers
                with torch.cuda.stream(engine.enc_stream):      # (on the encoder stream, ahead of the ingests that follow)
                    for b in engine.rt.enc_bufs:
                        b.img_in.zero_()
                self._zeroed_rt = engine.rt
            stage = self._buf('stage_enc', (la * P, int(src.shape[1]), int(src.shape[2]), 3), torch.uint8)
            self.ingest([(src, i, need[r], stage[r * la:], [dst[k * B + r] for k in range(need[r])]) for r, (src, i, _) in plan.items()], es)
            if self.flip:                                       # the twins' rows: the mirror of what was just ingested
                for k in range(max(need.values())):
                    self.mirror(dst[k * B:k * B + P], dst[k * B + P:(k + 1) * B], es)
        else:
            H, W = int(src.shape[-2]), int(src.shape[-1])
            table = lookahead_rows(plan, B, P, la, self.flip)
            if self.flip:
                # staging rows per look-ahead buffer: read by the encoder launch that follows, rewritten on this stream only after it
                st = self._buf('twin_stage', (2, P, la, 3, H, W), torch.float32)[buf]
                for r, (src, i, _) in plan.items():
                    self.mirror(src[i:i + need[r]], st[r, :need[r]], es)
            if len(plan) < P:
                with torch.cuda.stream(engine.enc_stream):      # zeroed on the only stream that reads it
                    idle = self._buf('idle_frame', (3, H, W), torch.float32, zero=True)
            enc.set_frames([plan[e[1]][0][e[2]] if e[0] == 'frame' else st[e[1], e[2]] if e[0] == 'twin' else idle for e in table], es)
        engine.encode_ahead(buf)
        return max(need.values())
