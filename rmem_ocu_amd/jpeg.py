"""Baseline JPEG frames decoded on the GPU (librmem_hip.so rmem_jpeg_*): compressed bytes in, the exact uint8 RGB Pillow
(libjpeg-turbo) produces out, [n, H, W, 3] on the device -- the layout rmem_ingest_rgb8 and the slots' uint8 path read.

    clip = JpegClip([open(p, 'rb').read() for p in paths])     # parsed + packed once into pinned memory
    rgb = decode(clip, device)                                  # uint8 [n, H, W, 3] device tensor

Supported: 8-bit baseline / extended Huffman, one scan, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart intervals optional,
any size.  Anything else raises RmemError with the reason (decode(..., host_fallback=True) decodes such files with Pillow).
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import JPEG_FORCE_FALLBACK, JpegDesc, JpegInfo as _CInfo, JpegPlan, RmemError

ST_COUNT, ST_CODE, ST_DESC = 1, 2, 4
CHUNK = 64          # decode() / evaluator.frames_from_jpegs decode at most this many frames per call (bounds the workspace)


@dataclass
class JpegInfo:
    width: int
    height: int
    components: int
    sampling: List[Tuple[int, int]]            # (h, v) per component, as written in SOF
    quant_ids: List[int]
    quantization: Dict[int, List[int]]         # table id -> 64 values in natural order (Pillow's im.quantization)
    restart_interval: int                      # MCUs, 0 = none
    scan_range: Tuple[int, int]                # entropy-coded segment [begin, end) in the file


def _as_bytes(data) -> bytes:
    return data if isinstance(data, bytes) else bytes(data)


def _parse_c(data: bytes) -> _CInfo:
    info = _CInfo()
    rc = _lib.lib().rmem_jpeg_parse(data, len(data), C.byref(info))
    if rc:
        raise RmemError(_lib.lib().rmem_last_error_string().decode())
    return info


def parse(data) -> JpegInfo:
    """Headers of one JPEG file (no GPU needed)."""
    i = _parse_c(_as_bytes(data))
    nc = i.components
    return JpegInfo(i.width, i.height, nc, [(i.h_samp[c], i.v_samp[c]) for c in range(nc)], [i.quant_id[c] for c in range(nc)],
                    {t: list(i.quant[t]) for t in range(4) if i.quant_mask >> t & 1}, i.restart_interval,
                    (i.scan_begin, i.scan_end))


class _DeviceCopy:
    """A packed clip on one device: the whole clip buffer's allocation (filled range by range), the descriptor table and a
    per-frame status word."""

    def __init__(self, packed: 'PackedJpegs', device):
        self.bits = torch.empty(max(packed.buf.numel(), 1), dtype=torch.uint8, device=device)
        self.descs = packed.desc_bytes.to(device)                      # once per clip and device
        self.status = torch.zeros(len(packed), dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()                # the zeroed status before any decode stream reads it

    def used_on(self, stream: torch.cuda.Stream):
        """these buffers are read / written on ``stream``: freeing the clip must not hand them out before it catches up"""
        for t in (self.bits, self.descs, self.status):
            t.record_stream(stream)


_WORKSPACES: Dict[Tuple[int, int], torch.Tensor] = {}
_PTR_TABLES: Dict[Tuple, torch.Tensor] = {}
_STREAMS: Dict[Tuple[int, int], torch.cuda.Stream] = {}


def _torch_stream(device, stream: int) -> torch.cuda.Stream:
    key = (device.index or 0, stream)
    st = _STREAMS.get(key)
    if st is None:
        st = _STREAMS[key] = torch.cuda.ExternalStream(stream, device=device)
    return st


# Device buffers that only the decode kernels touch are ALLOCATED ON THE STREAM THAT RUNS THOSE KERNELS: when one is dropped
# (a workspace grown, a pointer table evicted), the caching allocator hands its block back only to later allocations on that
# same stream, which run after the queued kernels that still read or write it.

def _workspace(device, stream: int, nbytes: int) -> torch.Tensor:
    """decode calls on one stream run in order, so they share one workspace"""
    key = (device.index or 0, stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        with torch.cuda.stream(_torch_stream(device, stream)):
            ws = _WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _ptr_table(device, stream: int, ptrs: Sequence[int]) -> torch.Tensor:
    """device int64 table of the output pointers (cached: the slots decode into the same staging rows every group)"""
    key = (device.index or 0, stream) + tuple(ptrs)
    t = _PTR_TABLES.get(key)
    if t is None:
        if len(_PTR_TABLES) > 4096:
            _PTR_TABLES.clear()
        with torch.cuda.stream(_torch_stream(device, stream)):      # copied in stream order from pinned memory: no host stall
            t = torch.tensor(list(ptrs), dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        _PTR_TABLES[key] = t
    return t


class PackedJpegs:
    """Frames parsed and packed once (rmem_jpeg_pack) into one pinned buffer plus a descriptor table; sizes may differ."""

    def __init__(self, frames: Sequence):
        datas = [_as_bytes(f) for f in frames]
        if not datas:
            raise RmemError('no JPEG frames')
        L = _lib.lib()
        infos = [_parse_c(d) for d in datas]
        total = sum(int(i.packed_bound) for i in infos) + 16
        pin = torch.cuda.is_available()                                # packing itself needs no GPU
        self.buf = torch.empty(total, dtype=torch.uint8, pin_memory=pin)
        descs = (JpegDesc * len(datas))()
        used = C.c_size_t(0)
        t0 = time.perf_counter()
        for k, d in enumerate(datas):
            if L.rmem_jpeg_pack(d, len(d), self.buf.data_ptr(), total, C.byref(used), C.byref(descs[k])):
                raise RmemError(f'frame {k}: {L.rmem_last_error_string().decode()}')
        self.pack_seconds = time.perf_counter() - t0
        self.descs = descs
        self.desc_bytes = torch.frombuffer(bytearray(descs), dtype=torch.uint8)
        if pin:
            self.desc_bytes = self.desc_bytes.pin_memory()
        self.offsets = [int(d.offset) for d in descs]
        self.ends = [int(d.offset + d.bytes) for d in descs]
        self.compressed_bytes = sum(len(d) for d in datas)
        self.sizes = [(int(d.height), int(d.width)) for d in descs]
        self._plans: Dict[int, JpegPlan] = {}
        self._dev: Dict[int, _DeviceCopy] = {}

    def __len__(self):
        return len(self.descs)

    def plan(self, batch: int) -> Tuple[JpegPlan, int]:
        """(plan, workspace bytes) for decoding up to ``batch`` of these frames per call"""
        if batch not in self._plans:
            p = JpegPlan()
            nb = _lib.lib().rmem_jpeg_workspace_bytes(self.descs, len(self.descs), batch, C.byref(p))
            if nb == 0:
                raise RmemError(_lib.lib().rmem_last_error_string().decode())
            self._plans[batch] = (p, int(nb))
        return self._plans[batch]

    def on_device(self, device) -> _DeviceCopy:
        device = torch.device(device)
        key = device.index or 0
        if key not in self._dev:
            self._dev[key] = _DeviceCopy(self, device)
        return self._dev[key]

    def upload(self, i: int, m: int, stream: int, device):
        """H2D copy of the compressed bytes of frames i .. i+m-1 (one contiguous range) on ``stream``"""
        dc = self.on_device(device)
        a, b = self.offsets[i], self.ends[i + m - 1]
        ops.copy_async(dc.bits[a:b], self.buf[a:b], b - a)(stream)

    def decode_into(self, outs: Sequence[torch.Tensor], i: int, m: int, stream: Optional[int] = None, *, upload: bool = True,
                    stats: Optional[torch.Tensor] = None, sync_rounds: Optional[int] = None, force_fallback: bool = False):
        """Decode frames i .. i+m-1 into outs[k] (uint8 [H_k, W_k, 3] contiguous device tensors) on ``stream``; the status
        words land in status()[i:i+m].  Asynchronous: nothing waits for the GPU."""
        assert len(outs) == m and 0 <= i and i + m <= len(self)
        device = outs[0].device
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        for k, o in enumerate(outs):
            h, w = self.sizes[i + k]
            if o.dtype != torch.uint8 or not o.is_cuda or not o.is_contiguous() or o.numel() != h * w * 3:
                raise RmemError(f'decode output {k}: expected a contiguous uint8 [{h}, {w}, 3] device tensor')
        plan, nbytes = self.plan(m)
        if sync_rounds is not None or force_fallback:
            plan = JpegPlan.from_buffer_copy(plan)
            if sync_rounds is not None:
                plan.sync_rounds = sync_rounds
            if force_fallback:
                plan.flags |= JPEG_FORCE_FALLBACK
        dc = self.on_device(device)
        if upload:
            self.upload(i, m, stream, device)
        ws = _workspace(device, stream, nbytes)
        ptrs = _ptr_table(device, stream, [o.data_ptr() for o in outs])
        dc.used_on(_torch_stream(device, stream))
        rc = _lib.lib().rmem_jpeg_decode_batch(dc.bits.data_ptr(), dc.descs.data_ptr(), i, m, C.byref(plan), ws.data_ptr(),
                                               ptrs.data_ptr(), dc.status.data_ptr() + 4 * i,
                                               None if stats is None else stats.data_ptr(), stream)
        _lib.check(rc, 'rmem_jpeg_decode_batch')

    def coefficients(self, device, i: int = 0, m: Optional[int] = None, *, sync_rounds: Optional[int] = None,
                     force_fallback: bool = False) -> List[torch.Tensor]:
        """Entropy decode only (rmem_jpeg_entropy_decode): int16 [total_blocks, 64] per frame, natural order, DC values,
        component planes back to back.  Synchronises."""
        device = torch.device(device)
        m = len(self) - i if m is None else m
        plan, nbytes = self.plan(m)
        plan = JpegPlan.from_buffer_copy(plan)
        if sync_rounds is not None:
            plan.sync_rounds = sync_rounds
        if force_fallback:
            plan.flags |= JPEG_FORCE_FALLBACK
        stream = torch.cuda.current_stream(device).cuda_stream
        dc = self.on_device(device)
        self.upload(i, m, stream, device)
        dc.used_on(torch.cuda.current_stream(device))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        rc = _lib.lib().rmem_jpeg_entropy_decode(dc.bits.data_ptr(), dc.descs.data_ptr(), i, m, C.byref(plan), ws.data_ptr(),
                                                 dc.status.data_ptr() + 4 * i, None, stream)
        _lib.check(rc, 'rmem_jpeg_entropy_decode')
        torch.cuda.current_stream(device).synchronize()
        out = []
        for k in range(m):
            nb = int(self.descs[i + k].total_blocks)
            a = k * plan.slot_bytes + plan.off_coef
            out.append(ws[a:a + nb * 128].view(torch.int16).view(nb, 64).clone())
        return out

    def status(self, device) -> torch.Tensor:
        return self.on_device(device).status

    def check(self, device, i: int = 0, m: Optional[int] = None, stream: Optional[int] = None):
        """Synchronise ``stream`` (the one the frames were decoded on; default: the current stream) and raise RmemError if a
        frame of i .. i+m-1 did not decode cleanly."""
        device = torch.device(device)
        m = len(self) - i if m is None else m
        if stream is not None:
            _torch_stream(device, stream).synchronize()
        st = self.status(device)[i:i + m].cpu()
        bad = torch.nonzero(st).flatten().tolist()
        if bad:
            k = bad[0]
            why = {ST_COUNT: 'block count', ST_CODE: 'invalid Huffman code', ST_DESC: 'descriptor outside the plan'}
            reasons = ', '.join(v for b, v in why.items() if int(st[k]) & b)
            raise RmemError(f'JPEG frame {i + k} failed to decode on the GPU (status {int(st[k])}: {reasons})'
                            + (f'; {len(bad)} frames bad' if len(bad) > 1 else ''))


class JpegClip(PackedJpegs):
    """The frames of one clip (equal sizes): what ClipSlot / GroupSlot.start accept in place of pinned uint8 frames.  The
    slots decode each look-ahead group straight into their uint8 staging rows."""

    dtype = torch.uint8

    def __init__(self, frames: Sequence):
        super().__init__(frames)
        if len(set(self.sizes)) != 1:
            raise RmemError(f'JpegClip: frames of one clip must share one size, got {sorted(set(self.sizes))}')
        h, w = self.sizes[0]
        self.shape = torch.Size((len(self), h, w, 3))

    def is_pinned(self) -> bool:
        return True


def decode(frames_or_bytes, device, stream: Optional[int] = None, check: bool = True, host_fallback: bool = False,
           stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [n, H, W, 3] device tensor of n equal-size JPEG frames (a JpegClip, or a sequence of bytes), decoded on ``stream``
    (default: the current stream) CHUNK frames per call.  check: synchronise that stream and raise RmemError on a non-zero
    status.  host_fallback: files the device decoder does not support are decoded with Pillow
    instead of raising.  stats: optional int32 device tensor [2] accumulating {sync launches that ran, units sent to the
    sequential fallback}."""
    device = torch.device(device)
    if isinstance(frames_or_bytes, (bytes, bytearray, memoryview)):
        frames_or_bytes = [frames_or_bytes]
    if isinstance(frames_or_bytes, PackedJpegs):
        clip = frames_or_bytes
    else:
        try:
            clip = JpegClip(frames_or_bytes)
        except RmemError:
            if not host_fallback:
                raise
            return _decode_on_host(frames_or_bytes, device)
    h, w = clip.sizes[0]
    if len(set(clip.sizes)) != 1:
        raise RmemError('decode: frames of different sizes (use PackedJpegs.decode_into)')
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    n = len(clip)
    with torch.cuda.stream(_torch_stream(device, stream)):
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=device)
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        clip.decode_into(list(out[k:k + m]), k, m, stream, stats=stats)
    if check:
        clip.check(device, stream=stream)
    return out


def _decode_on_host(frames, device) -> torch.Tensor:
    import io

    import numpy as np
    from PIL import Image
    arrs = [np.asarray(Image.open(io.BytesIO(_as_bytes(f))).convert('RGB')) for f in frames]
    return torch.from_numpy(np.stack(arrs)).to(device)
