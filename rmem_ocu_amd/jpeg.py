"""Baseline JPEG frames decoded on the GPU (librmem_hip.so rmem_jpeg_*): compressed bytes in, the exact uint8 RGB Pillow
(libjpeg-turbo) produces out, [n, H, W, 3] on the device -- the layout rmem_ingest_rgb8 and the slots' uint8 path read.

    clip = JpegClip([open(p, 'rb').read() for p in paths])     # parsed + packed once into pinned memory
    rgb = decode(clip, device)                                  # uint8 [n, H, W, 3] device tensor

Supported: 8-bit baseline / extended Huffman, one scan, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart intervals optional,
any size.  Anything else raises RmemError with the reason (decode(..., host_fallback=True) decodes such files with Pillow).

The other direction (rmem_jpeg_encode_rgb8, rmem_overlay_rgb8): uint8 RGB frames on the device, optionally with uint8 label maps
that are overlaid first (palette tint + black contour), out as complete baseline .jpg files (4:2:0, standard tables) whose
entropy-coded segment is libjpeg-turbo's byte for byte; only the compressed bytes cross to the host.

    files = encode_rgb_stack(rgb, labels, quality=90)           # one .jpg file (bytes) per frame
    evaluator.save_overlays(rgb, labels, paths)                 # the same, written to paths
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._codec import Packed, davis_palette, fetch_files, stream_of, uint8_stack, workspace
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


_PTR_TABLES: Dict[Tuple, torch.Tensor] = {}


def _ptr_table(device, stream: int, ptrs: Sequence[int]) -> torch.Tensor:
    """device int64 table of the output pointers (cached: the slots decode into the same staging rows every group)"""
    key = (device.index or 0, stream) + tuple(ptrs)
    t = _PTR_TABLES.get(key)
    if t is None:
        if len(_PTR_TABLES) > 4096:
            _PTR_TABLES.clear()
        with torch.cuda.stream(stream_of(device, stream)):          # copied in stream order from pinned memory: no host stall
            t = torch.tensor(list(ptrs), dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        _PTR_TABLES[key] = t
    return t


class PackedJpegs(Packed):
    """Frames parsed and packed once (rmem_jpeg_pack) into one pinned buffer plus a descriptor table; sizes may differ."""
    NOUN, STATUS_NAMES = 'JPEG', {ST_COUNT: 'block count', ST_CODE: 'invalid Huffman code', ST_DESC: 'descriptor outside the plan'}

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
        self._dev = {}

    def plan(self, batch: int) -> Tuple[JpegPlan, int]:
        """(plan, workspace bytes) for decoding up to ``batch`` of these frames per call"""
        if batch not in self._plans:
            p = JpegPlan()
            nb = _lib.lib().rmem_jpeg_workspace_bytes(self.descs, len(self.descs), batch, C.byref(p))
            if nb == 0:
                raise RmemError(_lib.lib().rmem_last_error_string().decode())
            self._plans[batch] = (p, int(nb))
        return self._plans[batch]

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
        ws = workspace('jpeg.decode', device, stream, nbytes)
        ptrs = _ptr_table(device, stream, [o.data_ptr() for o in outs])
        dc.used_on(stream_of(device, stream))
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

    def check(self, device, i: int = 0, m: Optional[int] = None, stream: Optional[int] = None):
        """Synchronise ``stream`` (the one the frames were decoded on; default: the current stream) and raise RmemError if a
        frame of i .. i+m-1 did not decode cleanly."""
        super().check(device, i, m, stream)


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
    with torch.cuda.stream(stream_of(device, stream)):
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


# ---------------------------------------------------------------------------------------------------------------- writing

_enc_tables: Dict[Tuple, torch.Tensor] = {}                # (device index, H, W, quality, restart_rows) -> device table blob
_enc_palettes: Dict[Tuple, torch.Tensor] = {}              # (device index, palette bytes or None) -> 768 device bytes


def _header_and_tables(H: int, W: int, quality: int, restart_rows: int) -> Tuple[bytes, np.ndarray]:
    for name, v in (('H', H), ('W', W), ('quality', quality), ('restart_rows', restart_rows)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not -2 ** 31 <= v < 2 ** 31:
            raise RmemError(f'jpeg.encode_header: {name} must be an integer (got {v!r})')
    header = (C.c_ubyte * _lib.JPEG_ENC_HEADER_MAX)()
    tables = np.zeros(_lib.JPEG_ENC_TABLE_BYTES, dtype=np.uint8)
    n = C.c_int(0)
    _lib.check(_lib.lib().rmem_jpeg_encode_header(int(H), int(W), int(quality), int(restart_rows), header, len(header), C.byref(n),
                                                  tables.ctypes.data), 'rmem_jpeg_encode_header')
    return bytes(header[:n.value]), tables


def encode_header(H: int, W: int, quality: int = 90, restart_rows: int = 1) -> bytes:
    """Everything of an encoded file before its entropy-coded segment: SOI, APP0 (JFIF 1.01), two DQT, SOF0 (4:2:0), four DHT,
    DRI (restart_rows MCU rows per interval; 0: none), SOS.  Host only; depends on nothing but its arguments."""
    return _header_and_tables(H, W, quality, restart_rows)[0]


def _device_tables(dev, H, W, quality, restart_rows) -> torch.Tensor:
    key = (dev.index, H, W, quality, restart_rows)
    t = _enc_tables.get(key)
    if t is None:
        if len(_enc_tables) > 256:
            _enc_tables.clear()
        t = _enc_tables[key] = torch.from_numpy(_header_and_tables(H, W, quality, restart_rows)[1]).to(dev)
    return t


def _device_palette(dev, palette) -> torch.Tensor:
    key = (dev.index, None if palette is None else bytes(bytearray(int(v) & 255 for v in palette)))
    t = _enc_palettes.get(key)
    if t is None:
        data = bytes(bytearray(davis_palette())) if key[1] is None else key[1]
        if len(data) != 768:
            raise RmemError(f'jpeg: the palette must have 256 RGB entries (got {len(data)} values)')
        if len(_enc_palettes) > 64:
            _enc_palettes.clear()
        t = _enc_palettes[key] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    return t


def _alpha256(alpha) -> int:
    a = int(round(256 * float(alpha)))
    if not 0 <= a <= 256:
        raise RmemError(f'jpeg: alpha must be in 0..1 (got {alpha})')
    return a


def _frames_and_labels(rgb_u8, labels_u8, what):
    """-> (rgb [n, H, W, 3], labels [n, H, W] or None); views only, nothing copied"""
    if not isinstance(rgb_u8, torch.Tensor) or rgb_u8.dtype != torch.uint8 or not rgb_u8.is_cuda:
        raise RmemError(f'{what}: rgb must be a uint8 device tensor')
    if rgb_u8.dim() not in (3, 4) or rgb_u8.shape[-1] != 3 or rgb_u8.numel() == 0:
        raise RmemError(f'{what}: rgb must be a non-empty [n, H, W, 3] or [H, W, 3] stack (got {tuple(rgb_u8.shape)})')
    rgb = rgb_u8[None] if rgb_u8.dim() == 3 else rgb_u8
    if labels_u8 is None:
        return rgb, None
    labels = uint8_stack(labels_u8, what)
    if labels.device != rgb.device:
        raise RmemError(f'{what}: rgb is on {rgb.device} but labels on {labels.device}')
    if tuple(labels.shape) != tuple(rgb.shape[:3]):
        raise RmemError(f'{what}: labels must be [n, H, W] matching rgb {tuple(rgb.shape)} (got {tuple(labels_u8.shape)})')
    return rgb, labels


def overlay(rgb_u8: torch.Tensor, labels_u8: torch.Tensor, alpha: float = 0.4, palette: Optional[Sequence[int]] = None) -> torch.Tensor:
    """uint8 [n, H, W, 3]: the frames with every object tinted in its palette colour (out = (a rgb + (256 - a) colour + 128) >> 8,
    a = round(256 alpha)) and a black one-pixel contour just outside it (a pixel one of whose 4-neighbours carries a larger label).
    palette: 768 values, default the DAVIS palette.  Enqueued on the current stream, no host sync."""
    if labels_u8 is None:
        raise RmemError('jpeg.overlay: labels must be a uint8 device tensor')
    rgb, labels = _frames_and_labels(rgb_u8, labels_u8, 'jpeg.overlay')
    rgb, labels = rgb.contiguous(), labels.contiguous()
    n, H, W, _ = rgb.shape
    dev = rgb.device
    a, pal = _alpha256(alpha), _device_palette(dev, palette)
    out = torch.empty_like(rgb)
    _lib.check(_lib.lib().rmem_overlay_rgb8(rgb.data_ptr(), labels.data_ptr(), pal.data_ptr(), a, n, H, W, out.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), 'rmem_overlay_rgb8')
    return out


def encode_files(rgb_u8: torch.Tensor, labels_u8: Optional[torch.Tensor] = None, quality: int = 90, restart_rows: int = 1,
                 alpha: float = 0.4, palette: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One complete .jpg file per frame of a uint8 device stack [n, H, W, 3] or [H, W, 3] (a non-contiguous view is copied first):
    returns (out, offsets), device tensors; file f is out[offsets[f]:offsets[f + 1]] (offsets: int64 [n + 1]), out is sized for
    the worst case n * rmem_jpeg_encode_bound(H, W).  labels_u8 ([n, H, W] or [H, W]): `overlay` is applied to the pixels as the
    encoder reads them.  Enqueued on the current stream, no host sync (the table blob of a new (H, W, quality, restart_rows) is
    uploaded once).  The workspace is one buffer per (device, stream) that only grows."""
    rgb, labels = _frames_and_labels(rgb_u8, labels_u8, 'jpeg.encode_files')
    rgb = rgb.contiguous()
    labels = None if labels is None else labels.contiguous()
    n, H, W, _ = rgb.shape
    dev = rgb.device
    tables = _device_tables(dev, H, W, quality, restart_rows)          # refuses bad geometry, quality and restart_rows by name
    a, pal = _alpha256(alpha), (None if labels is None else _device_palette(dev, palette))
    L = _lib.lib()
    bound, nbytes = L.rmem_jpeg_encode_bound(H, W), L.rmem_jpeg_encode_workspace_bytes(n, H, W)
    if bound == 0 or nbytes == 0:
        raise RmemError(f'jpeg.encode_files: bad geometry {n} x {H}x{W}')
    stream = torch.cuda.current_stream(dev)
    ws = workspace('jpeg.encode', dev, stream, nbytes)
    out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.check(L.rmem_jpeg_encode_rgb8(rgb.data_ptr(), None if labels is None else labels.data_ptr(),
                                       None if pal is None else pal.data_ptr(), a, n, H, W, tables.data_ptr(), ws.data_ptr(),
                                       out.data_ptr(), offsets.data_ptr(), stream.cuda_stream), 'rmem_jpeg_encode_rgb8')
    return out, offsets


def encode_rgb_stack(rgb_u8: torch.Tensor, labels_u8: Optional[torch.Tensor] = None, quality: int = 90, restart_rows: int = 1,
                     alpha: float = 0.4, palette: Optional[Sequence[int]] = None) -> List[bytes]:
    """Complete .jpg files (bytes), one per frame.  Per chunk of at most CHUNK frames: one encode call, then two device-to-host
    copies into pinned memory -- the offsets, then the offsets[n] bytes of the files."""
    rgb, labels = _frames_and_labels(rgb_u8, labels_u8, 'jpeg.encode_rgb_stack')
    n = rgb.shape[0]
    dev = rgb.device
    stream = torch.cuda.current_stream(dev)
    files: List[bytes] = []
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        out, offsets = encode_files(rgb[k:k + m], None if labels is None else labels[k:k + m], quality, restart_rows, alpha, palette)
        files += fetch_files(out, offsets, m, stream, 'jpeg.encode_rgb_stack')
    return files
