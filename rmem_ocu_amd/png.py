"""Predicted label maps -> indexed PNG files, the DEFLATE payload encoded on the device (rmem_png_encode_labels, include/rmem.h).

Replaces the Pillow encoder inside evaluator.save_mask (utils/image.py:90-106) for stacks of masks: the labels stay on the device,
one call encodes every frame of a stack into a zlib stream of a fixed-Huffman, run-length-only format, and only those streams (a
few KB per frame instead of H * W bytes) cross to the host, where `wrap` adds the PNG chunks.  The chunk CRC-32s are computed here
on the host with zlib.crc32: they run over a few KB per frame.

    files = png.encode_label_stack(slot.labels[c, 1:n])            # after engine.synchronize(): one PNG file (bytes) per frame
    evaluator.save_masks(slot.labels[c, 1:n], paths, squeeze_idx)  # the same, written to paths
"""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

CHUNK = 64                                                 # frames per encode call of encode_label_stack
_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_ws: Dict[Tuple[int, int], torch.Tensor] = {}              # (device index, stream) -> row bits / Adler partials, grow-only
_pinned: Dict[int, List[torch.Tensor]] = {}                # device index -> [offsets, bytes] pinned host buffers, grow-only


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def wrap(zlib_stream: bytes, H: int, W: int, palette: Optional[Sequence[int]] = None) -> bytes:
    """A complete PNG file around one frame's zlib stream: signature, IHDR (8 bit, colour type 3 = indexed), PLTE (256 entries, the
    DAVIS palette unless `palette` gives 768 values), IDAT, IEND.  Pure host code."""
    if palette is None:
        from .evaluator import _davis_palette
        palette = _davis_palette()
    pal = bytes(bytearray(int(v) & 255 for v in palette))
    if len(pal) != 768:
        raise _lib.RmemError(f'png.wrap: the palette must have 256 RGB entries (got {len(pal)} values)')
    if H < 1 or W < 1:
        raise _lib.RmemError(f'png.wrap: bad size {H}x{W}')
    return (_SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', int(W), int(H), 8, 3, 0, 0, 0)) + _chunk(b'PLTE', pal)
            + _chunk(b'IDAT', bytes(zlib_stream)) + _chunk(b'IEND', b''))


def squeeze_lut(squeeze_idx: Sequence[int]) -> np.ndarray:
    """save_mask's un-squeeze as a 256-entry table: entry i = squeeze_idx[i] for 1 <= i < len(squeeze_idx), every other entry 0."""
    lut = np.zeros(256, dtype=np.uint8)
    for i in range(1, min(len(squeeze_idx), 256)):
        lut[i] = int(squeeze_idx[i]) & 255
    return lut


def _stack(labels_u8, what):
    if not isinstance(labels_u8, torch.Tensor) or labels_u8.dtype != torch.uint8 or not labels_u8.is_cuda:
        raise _lib.RmemError(f'{what}: labels must be a uint8 device tensor')
    if labels_u8.dim() not in (2, 3) or labels_u8.numel() == 0:
        raise _lib.RmemError(f'{what}: labels must be a non-empty [n, H, W] or [H, W] stack (got {tuple(labels_u8.shape)})')
    return labels_u8[None] if labels_u8.dim() == 2 else labels_u8


def encode_zlib(labels_u8: torch.Tensor, lut: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One zlib stream per frame of a uint8 device label stack [n, H, W] or [H, W] (a non-contiguous view is copied first):
    returns (out, offsets), device tensors; stream f is out[offsets[f]:offsets[f + 1]] (offsets: int64 [n + 1]), out is sized for the
    worst case n * rmem_png_zlib_bound(H, W).  lut: 256 uint8 device values applied to every label, or None.  Enqueued on the current
    stream, no host sync.  The workspace is one buffer per (device, stream) that only grows."""
    labels = _stack(labels_u8, 'png.encode_zlib').contiguous()
    n, H, W = labels.shape
    dev = labels.device
    if lut is not None and (not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.device != dev or lut.numel() != 256
                            or not lut.is_contiguous()):
        raise _lib.RmemError('png.encode_zlib: lut must be 256 contiguous uint8 values on the labels\' device')
    L = _lib.lib()
    bound, nbytes = L.rmem_png_zlib_bound(H, W), L.rmem_png_workspace_bytes(n, H, W)
    if bound == 0 or nbytes == 0:
        raise _lib.RmemError(f'png.encode_zlib: frame too large (H * W must not exceed 2^26, got {H}x{W})')
    stream = torch.cuda.current_stream(dev)
    key = (dev.index, stream.cuda_stream)
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:
        with torch.cuda.stream(stream):
            ws = _ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.check(L.rmem_png_encode_labels(labels.data_ptr(), n, H, W, None if lut is None else lut.data_ptr(), ws.data_ptr(),
                                        out.data_ptr(), offsets.data_ptr(), stream.cuda_stream), 'rmem_png_encode_labels')
    return out, offsets


def _pinned_buffers(dev_index: int, nbytes: int, noffsets: int) -> List[torch.Tensor]:
    bufs = _pinned.get(dev_index)
    if bufs is None:
        bufs = _pinned[dev_index] = [torch.empty(CHUNK + 1, dtype=torch.int64).pin_memory(), torch.empty(0, dtype=torch.uint8)]
    if bufs[0].numel() < noffsets:
        bufs[0] = torch.empty(noffsets, dtype=torch.int64).pin_memory()
    if bufs[1].numel() < nbytes:
        bufs[1] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    return bufs


def encode_label_stack(labels_u8: torch.Tensor, squeeze_idx: Optional[Sequence[int]] = None,
                       palette: Optional[Sequence[int]] = None) -> List[bytes]:
    """Complete PNG files (bytes), one per frame of a uint8 device label stack [n, H, W] or [H, W].  Per chunk of at most CHUNK
    frames: one encode call, then exactly two device-to-host copies into pinned memory -- the offsets, then the offsets[n] bytes
    of the streams -- and `wrap` on the host.  squeeze_idx: save_mask's un-squeeze, applied on the device as a table."""
    labels = _stack(labels_u8, 'png.encode_label_stack')
    n, H, W = labels.shape
    dev = labels.device
    stream = torch.cuda.current_stream(dev)
    lut = None if squeeze_idx is None else torch.from_numpy(squeeze_lut(squeeze_idx)).to(dev)
    files: List[bytes] = []
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        out, offsets = encode_zlib(labels[k:k + m], lut)
        off_h, _ = _pinned_buffers(dev.index, 0, m + 1)
        off_h[:m + 1].copy_(offsets, non_blocking=True)
        stream.synchronize()
        off = off_h[:m + 1].tolist()
        total = off[m]
        if off[0] != 0 or total > out.numel() or any(b <= a for a, b in zip(off, off[1:])):
            raise _lib.RmemError(f'png.encode_label_stack: bad stream offsets from the device ({off[:4]} ... {total})')
        _, data_h = _pinned_buffers(dev.index, total, m + 1)
        data_h[:total].copy_(out[:total], non_blocking=True)
        stream.synchronize()
        data = data_h[:total].numpy().tobytes()
        files += [wrap(data[off[i]:off[i + 1]], H, W, palette) for i in range(m)]
    return files
