"""Palette PNGs on the device, both directions.

Writing: predicted label maps -> indexed PNG files, the DEFLATE payload encoded on the device (rmem_png_encode_labels, include/rmem.h).

Replaces the Pillow encoder inside evaluator.save_mask (utils/image.py:90-106) for stacks of masks: the labels stay on the device,
one call encodes every frame of a stack into a zlib stream of a fixed-Huffman, run-length-only format, and only those streams (a
few KB per frame instead of H * W bytes) cross to the host, where `wrap` adds the PNG chunks.  The chunk CRC-32s are computed here
on the host with zlib.crc32: they run over a few KB per frame.

    files = png.encode_label_stack(slot.labels[c, 1:n])            # after engine.synchronize(): one PNG file (bytes) per frame
    evaluator.save_masks(slot.labels[c, 1:n], paths, squeeze_idx)  # the same, written to paths

Reading: annotation files -> uint8 label maps on the device (rmem_png_decode_labels).  Replaces Image.open of an annotation in
dataloaders/eval_datasets.py: `parse` walks the chunks and checks their CRC-32s on the host (a few KB per file), PackedPngs packs the
zlib streams of a clip's files into one pinned buffer, and only those bytes cross to the device, where they are inflated,
unfiltered, unpacked and (optionally) mapped through a 256-entry table.

    gt = png.decode_label_stack(paths, device)                      # uint8 [n, H, W], Pillow's np.array(Image.open(p)) bit for bit
    gt = evaluator.labels_from_pngs(paths, device)                  # the same
"""
from __future__ import annotations

import struct
import zlib
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import Packed, davis_palette, fetch_files, stream_of, uint8_stack, workspace

CHUNK = 64                                                 # frames per encode call of encode_label_stack
_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def wrap(zlib_stream: bytes, H: int, W: int, palette: Optional[Sequence[int]] = None) -> bytes:
    """A complete PNG file around one frame's zlib stream: signature, IHDR (8 bit, colour type 3 = indexed), PLTE (256 entries, the
    DAVIS palette unless `palette` gives 768 values), IDAT, IEND.  Pure host code."""
    pal = bytes(bytearray(int(v) & 255 for v in (davis_palette() if palette is None else palette)))
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


def encode_zlib(labels_u8: torch.Tensor, lut: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One zlib stream per frame of a uint8 device label stack [n, H, W] or [H, W] (a non-contiguous view is copied first):
    returns (out, offsets), device tensors; stream f is out[offsets[f]:offsets[f + 1]] (offsets: int64 [n + 1]), out is sized for the
    worst case n * rmem_png_zlib_bound(H, W).  lut: 256 uint8 device values applied to every label, or None.  Enqueued on the current
    stream, no host sync.  The workspace is one buffer per (device, stream) that only grows."""
    labels = uint8_stack(labels_u8, 'png.encode_zlib').contiguous()
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
    ws = workspace('png.encode', dev, stream, nbytes)           # row bits / Adler partials
    out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.check(L.rmem_png_encode_labels(labels.data_ptr(), n, H, W, None if lut is None else lut.data_ptr(), ws.data_ptr(),
                                        out.data_ptr(), offsets.data_ptr(), stream.cuda_stream), 'rmem_png_encode_labels')
    return out, offsets


def encode_label_stack(labels_u8: torch.Tensor, squeeze_idx: Optional[Sequence[int]] = None,
                       palette: Optional[Sequence[int]] = None) -> List[bytes]:
    """Complete PNG files (bytes), one per frame of a uint8 device label stack [n, H, W] or [H, W].  Per chunk of at most CHUNK
    frames: one encode call, then exactly two device-to-host copies into pinned memory -- the offsets, then the offsets[n] bytes
    of the streams -- and `wrap` on the host.  squeeze_idx: save_mask's un-squeeze, applied on the device as a table."""
    labels = uint8_stack(labels_u8, 'png.encode_label_stack')
    n, H, W = labels.shape
    dev = labels.device
    stream = torch.cuda.current_stream(dev)
    lut = None if squeeze_idx is None else torch.from_numpy(squeeze_lut(squeeze_idx)).to(dev)
    files: List[bytes] = []
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        out, offsets = encode_zlib(labels[k:k + m], lut)
        files += [wrap(z, H, W, palette) for z in fetch_files(out, offsets, m, stream, 'png.encode_label_stack')]
    return files


# ---------------------------------------------------------------------------------------------------------------- reading

ST_INPUT, ST_SIZE, ST_RANGE, ST_CODE, ST_HEADER, ST_ADLER, ST_FILTER, ST_DESC = 1, 2, 4, 8, 16, 32, 64, 128    # include/rmem.h
STATUS_NAMES = {ST_INPUT: 'the stream ends too early', ST_SIZE: 'wrong number of inflated bytes', ST_RANGE: 'distance too far back',
                ST_CODE: 'invalid block or code', ST_HEADER: 'bad zlib header', ST_ADLER: 'Adler-32 mismatch',
                ST_FILTER: 'filter type above 4', ST_DESC: 'bad descriptor'}
MAX_PIXELS = 1 << 26


class PngUnsupported(_lib.RmemError):
    """A well-formed PNG file in a format the device decoder refuses (decode_label_stack(host_fallback=True) hands these, and only
    these, to Pillow)."""


@dataclass
class PngInfo:
    width: int
    height: int
    bit_depth: int
    colour_type: int
    interlace: int
    palette: Optional[bytes]                   # the PLTE payload (3 bytes per entry), or None
    idat_ranges: List[Tuple[int, int]]         # [begin, end) of every IDAT payload in the file

    def refusal(self) -> Optional[str]:
        """why the device decoder does not take this file, or None"""
        if self.interlace:
            return 'interlaced PNG'
        if self.bit_depth == 16:
            return '16-bit samples'
        if self.colour_type in (2, 4, 6):
            return f'colour type {self.colour_type} (only indexed and 8-bit grey are decoded)'
        if self.colour_type == 0 and self.bit_depth != 8:
            return f'grey at bit depth {self.bit_depth} (only 8)'
        if self.colour_type not in (0, 3) or self.bit_depth not in (1, 2, 4, 8):
            return f'colour type {self.colour_type} at bit depth {self.bit_depth}'
        if self.width * self.height > MAX_PIXELS:
            return f'frame too large (H * W must not exceed 2^26, got {self.height}x{self.width})'
        return None


def _read(f) -> bytes:
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    with open(f, 'rb') as fh:
        return fh.read()


def parse(data, check: bool = True) -> PngInfo:
    """The chunks of one PNG file (no GPU needed): every chunk's CRC-32 is verified here.  A damaged file raises RmemError with the
    reason; a sound file in a format the device decoder refuses raises PngUnsupported unless check is False."""
    data = _read(data)
    if data[:8] != _SIGNATURE:
        raise _lib.RmemError('png.parse: bad signature (not a PNG file)')
    at, ihdr, palette, idat, end = 8, None, None, [], False
    while at < len(data) and not end:
        if at + 12 > len(data):
            raise _lib.RmemError(f'png.parse: truncated chunk header at byte {at}')
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        if at + 12 + n > len(data):
            raise _lib.RmemError(f'png.parse: chunk {kind!r} at byte {at} runs past the end of the file')
        body = data[at + 8:at + 8 + n]
        if zlib.crc32(data[at + 4:at + 8 + n]) & 0xFFFFFFFF != struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0]:
            raise _lib.RmemError(f'png.parse: chunk CRC mismatch in {kind!r} at byte {at}')
        if ihdr is None and kind != b'IHDR':
            raise _lib.RmemError('png.parse: missing IHDR (it must be the first chunk)')
        if kind == b'IHDR':
            if n != 13:
                raise _lib.RmemError('png.parse: IHDR must have 13 bytes')
            ihdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'PLTE':
            palette = body
        elif kind == b'IDAT':
            idat.append((at + 8, at + 8 + n))
        elif kind == b'IEND':
            end = True
        at += 12 + n                                    # every other chunk is ancillary here: skipped
    if ihdr is None:
        raise _lib.RmemError('png.parse: missing IHDR')
    if not idat:
        raise _lib.RmemError('png.parse: missing IDAT')
    if not end:
        raise _lib.RmemError('png.parse: missing IEND')
    w, h, depth, ctype, comp, filt, interlace = ihdr
    if w < 1 or h < 1 or comp != 0 or filt != 0 or interlace > 1 or (ctype, depth) not in {
            (0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)}:
        raise _lib.RmemError(f'png.parse: invalid IHDR {ihdr}')
    info = PngInfo(w, h, depth, ctype, interlace, palette, idat)
    if check and info.refusal():
        raise PngUnsupported(f'png.parse: {info.refusal()}')
    return info


class PackedPngs(Packed):
    """Annotation files (paths or bytes) of one size, parsed once: the IDAT payloads of every file concatenated into its zlib
    stream, the streams packed back to back into one pinned buffer -- each 8-byte aligned and followed by at least 8 zero bytes --
    and the descriptor table (RmemPngDesc).  Bit depth and colour type may differ per frame."""
    NOUN, STATUS_NAMES = 'PNG', STATUS_NAMES

    def __init__(self, files: Sequence):
        datas = [_read(f) for f in files]
        if not datas:
            raise _lib.RmemError('PackedPngs: no files')
        self.infos = [parse(d) for d in datas]
        sizes = sorted({(i.height, i.width) for i in self.infos})
        if len(sizes) != 1:
            raise _lib.RmemError(f'PackedPngs: frames of one pack must share one size, got {sizes}')
        self.height, self.width = sizes[0]
        self.shape = torch.Size((len(datas), self.height, self.width))
        streams = [b''.join(d[a:b] for a, b in i.idat_ranges) for d, i in zip(datas, self.infos)]
        self.descs = (_lib.PngDesc * len(datas))()
        at = 0
        for k, (st, i) in enumerate(zip(streams, self.infos)):
            self.descs[k] = _lib.PngDesc(at, len(st), i.bit_depth, i.colour_type)
            at += (len(st) + 8 + 7) & ~7
        host = np.zeros(at, dtype=np.uint8)
        for d, st in zip(self.descs, streams):
            host[d.offset:d.offset + len(st)] = np.frombuffer(st, dtype=np.uint8)
        pin = torch.cuda.is_available()                                # packing itself needs no GPU
        self.buf = torch.from_numpy(host)
        self.desc_bytes = torch.frombuffer(bytearray(self.descs), dtype=torch.uint8)
        if pin:
            self.buf, self.desc_bytes = self.buf.pin_memory(), self.desc_bytes.pin_memory()
        self.offsets = [int(d.offset) for d in self.descs]
        self.ends = self.offsets[1:] + [at]                            # a frame's range includes its padding
        self.palettes = [i.palette for i in self.infos]
        self.compressed_bytes = sum(len(st) for st in streams)
        self._dev = {}


def _device_lut(lut, dev, what) -> Optional[torch.Tensor]:
    if lut is None:
        return None
    if not isinstance(lut, torch.Tensor):
        arr = np.asarray(lut)
        if arr.dtype != np.uint8 or arr.shape != (256,):
            raise _lib.RmemError(f'{what}: lut must be 256 contiguous uint8 values')
        return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    if lut.dtype != torch.uint8 or lut.numel() != 256 or lut.dim() != 1 or not lut.is_contiguous() or lut.device != dev:
        raise _lib.RmemError(f'{what}: lut must be 256 contiguous uint8 values on the output\'s device')
    return lut


def decode_labels_into(packed: PackedPngs, out: torch.Tensor, first: int = 0, count: Optional[int] = None, stream=None, lut=None):
    """Frames first .. first+count-1 of `packed` into out (uint8 [count, H, W], contiguous, device) on ``stream`` (a
    torch.cuda.Stream or a raw handle; default: the current stream).  Nothing waits for the GPU: the compressed bytes are copied
    from pinned memory on the stream, the status words land in packed.status(device)[first:first+count] and are read later by
    packed.check(device).  The workspace is one buffer per (device, stream) that only grows, allocated on that stream."""
    count = len(packed) - first if count is None else count
    if not isinstance(packed, PackedPngs) or not 0 <= first or count < 1 or first + count > len(packed):
        raise _lib.RmemError(f'png.decode_labels_into: frames {first}..{first + count - 1} of {len(packed)}')
    H, W = packed.height, packed.width
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda:
        raise _lib.RmemError('png.decode_labels_into: out must be a uint8 device tensor')
    if tuple(out.shape) != (count, H, W) or not out.is_contiguous():
        raise _lib.RmemError(f'png.decode_labels_into: out must be a contiguous [{count}, {H}, {W}] tensor (got {tuple(out.shape)})')
    dev = out.device
    lut = _device_lut(lut, dev, 'png.decode_labels_into')
    ts = stream_of(dev, stream)
    L = _lib.lib()
    nbytes = L.rmem_png_decode_workspace_bytes(count, H, W)
    if nbytes == 0:
        raise _lib.RmemError(f'png.decode_labels_into: frame too large (H * W must not exceed 2^26, got {H}x{W})')
    dc = packed.on_device(dev)
    ws = workspace('png.decode', dev, ts, nbytes)               # the inflated bytes
    dc.used_on(ts)
    for t in (out,) + (() if lut is None else (lut,)):
        t.record_stream(ts)
    a, b = packed.offsets[first], packed.ends[first + count - 1]
    from . import ops
    ops.copy_async(dc.bits[a:b], packed.buf[a:b], b - a)(ts.cuda_stream)
    _lib.check(L.rmem_png_decode_labels(dc.bits.data_ptr(), dc.descs.data_ptr() + C.sizeof(_lib.PngDesc) * first, count, H, W,
                                        None if lut is None else lut.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                        dc.status.data_ptr() + 4 * first, ts.cuda_stream), 'rmem_png_decode_labels')


def _host_label(data: bytes) -> np.ndarray:
    import io

    from PIL import Image
    arr = np.array(Image.open(io.BytesIO(data)))                       # palette indices, not RGB
    if arr.ndim != 2 or arr.min() < 0 or arr.max() > 255:
        raise _lib.RmemError(f'png.decode_label_stack: not a label map (Pillow gives shape {arr.shape}, dtype {arr.dtype})')
    return arr.astype(np.uint8)


def decode_label_stack(files_or_packed, device, lut=None, host_fallback: bool = False) -> torch.Tensor:
    """uint8 [n, H, W] label maps on `device` of n annotation files of one size (paths, bytes, or a PackedPngs): what
    np.array(Image.open(f)) gives per file, bit for bit, through `lut` (256 uint8 values) if given.  At most CHUNK frames per
    decode call; after the last one, one synchronisation and one readback of the status words: a non-zero word raises RmemError
    naming the frame and the bits.  host_fallback: files in a format the device decoder refuses (not damaged ones) are decoded by
    Pillow and uploaded instead of raising PngUnsupported."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.RmemError('png.decode_label_stack: the target must be a GPU device (there is no host decoder)')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    lut = _device_lut(lut, device, 'png.decode_label_stack')
    if isinstance(files_or_packed, (bytes, bytearray, memoryview, str)):
        files_or_packed = [files_or_packed]
    host: Dict[int, np.ndarray] = {}
    if isinstance(files_or_packed, PackedPngs):
        packed, n, on_dev = files_or_packed, len(files_or_packed), list(range(len(files_or_packed)))
    else:
        datas = [_read(f) for f in files_or_packed]
        n = len(datas)
        if host_fallback:
            for k, d in enumerate(datas):
                try:
                    parse(d)
                except PngUnsupported:
                    host[k] = _host_label(d)
        on_dev = [k for k in range(n) if k not in host]
        packed = PackedPngs([datas[k] for k in on_dev]) if on_dev else None
    if packed is not None:
        H, W = packed.height, packed.width
    else:
        H, W = next(iter(host.values())).shape
    if any(a.shape != (H, W) for a in host.values()):
        raise _lib.RmemError('png.decode_label_stack: frames of one stack must share one size')
    stream = torch.cuda.current_stream(device)
    out = torch.empty(n, H, W, dtype=torch.uint8, device=device)
    dec = out if not host else torch.empty(len(on_dev), H, W, dtype=torch.uint8, device=device)
    for k in range(0, len(on_dev), CHUNK):
        m = min(CHUNK, len(on_dev) - k)
        decode_labels_into(packed, dec[k:k + m], k, m, stream, lut)
    if host:
        if on_dev:
            out[torch.tensor(on_dev, device=device)] = dec
        up = torch.from_numpy(np.stack([host[k] for k in sorted(host)])).to(device)
        out[torch.tensor(sorted(host), device=device)] = up if lut is None else lut[up.long()]
    if packed is not None:
        packed.check(device, 0, len(on_dev), stream)
    return out
