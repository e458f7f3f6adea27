"""COCO run-length masks ({'size': [H, W], 'counts': ...}) on the device, both directions.

The format of BURST / TAO-VOS annotations and submissions, YouTube-VIS / OVIS results, SA-V masklets and everything that goes
through pycocotools: a binary mask read column-major, the lengths of its alternating runs (zeros first), written as 5-bit groups
in the characters 48..111 (include/rmem.h restates maskApi.c).

Writing: predicted label maps -> one string per frame and object, built on the device (rmem_rle_encode_labels).  Replaces
stack.cpu() and pycocotools' encode per frame and object: the labels stay on the device, only the strings (a few hundred bytes per
mask, typically) cross to the host.

    per_frame = rle.encode_label_stack(slot.labels[c, 1:n], num_ids)         # [{object id: {'size': [H, W], 'counts': bytes}}]
    per_frame = evaluator.rle_results(labels, num_objs, proto.squeeze_idx)   # the same with str counts, ready for json.dump

Reading: annotation strings -> uint8 label maps on the device (rmem_rle_decode_labels).  Replaces pycocotools' decode per mask
and the upload of H * W bytes per frame: PackedRles packs a clip's strings into one pinned buffer with a descriptor table, only
those bytes cross to the device.

    gt = rle.decode_label_stack(frames, (H, W), device)                      # frames[f] = {label value: rle}; uint8 [n, H, W]
    gt, ids = evaluator.labels_from_rles(frames, (H, W), device)             # frames[f] = {track id: rle}; value i + 1 = ids[i]
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import Packed, fetch_files, stream_of, uint8_stack, workspace
from ._labels import object_keys

# encode_label_stack gives one encode call as many frames as keep rmem_rle_workspace_bytes at or below this (one frame at least,
# MAX_FRAMES at most): per frame 8 H W bytes of boundary positions plus 4 * num_ids * W * ceil(H / 128) bytes of counters.
WORKSPACE_CAP = 256 << 20
MAX_FRAMES = 1024
MAX_PIXELS = 1 << 26
ST_CAPACITY = 1                                                     # include/rmem.h
ST_CHAR, ST_TRUNCATED, ST_LONG, ST_NEGATIVE, ST_SUM, ST_DESC = 1, 2, 4, 8, 16, 32
STATUS_NAMES = {ST_CHAR: 'a byte outside 48..111', ST_TRUNCATED: 'the string ends inside a count', ST_LONG: 'a count of more than 6 characters',
                ST_NEGATIVE: 'a count below 0', ST_SUM: 'the counts do not add up to H * W', ST_DESC: 'bad descriptor'}


def default_capacity(frames: int, H: int, W: int, num_ids: int) -> int:
    """The bytes `encode` gives `out` when the caller names none: 16 per string plus one per 8 pixels of every frame.  An estimate,
    not a bound -- a checkerboard needs about one byte per pixel: blob-like masks of a few hundred bytes each fit many times over,
    and when the strings do not fit, the status word says so and the offsets still give the exact size."""
    return frames * (16 * num_ids + (H * W + 7) // 8)


def frames_per_call(H: int, W: int, num_ids: int) -> int:
    """how many frames one encode call of encode_label_stack takes (WORKSPACE_CAP, MAX_FRAMES)"""
    per = _lib.lib().rmem_rle_workspace_bytes(1, H, W, num_ids)
    if per == 0:
        raise _lib.RmemError(f'rle: bad geometry (H * W must not exceed 2^26, num_ids must be in 1..255; got {H}x{W}, {num_ids})')
    return max(1, min(MAX_FRAMES, WORKSPACE_CAP // per))


def encode(labels_u8: torch.Tensor, num_ids: int, capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One string per (frame, id), id = 1..num_ids, of a uint8 device label stack [n, H, W] or [H, W] (a non-contiguous view is
    copied first): returns (out, offsets, status), device tensors.  String (f, k) is out[offsets[f * num_ids + k - 1] :
    offsets[f * num_ids + k]] (offsets: int64 [n * num_ids + 1]); out holds `capacity` bytes (default_capacity when None).  status
    (int32 [1]) is ST_CAPACITY when the strings need more: out is untouched then and offsets is still exact.  One call, enqueued on
    the current stream, no host sync; the workspace (whatever its size: callers with long stacks chunk as encode_label_stack
    does) is one buffer per (device, stream) that only grows."""
    labels = uint8_stack(labels_u8, 'rle.encode').contiguous()
    n, H, W = labels.shape
    dev = labels.device
    K = int(num_ids)
    L = _lib.lib()
    nbytes = L.rmem_rle_workspace_bytes(n, H, W, K)
    if nbytes == 0:
        raise _lib.RmemError(f'rle.encode: bad geometry (at most 65535 frames, H * W at most 2^26, num_ids in 1..255; got {n}x{H}x{W}, {num_ids})')
    cap = default_capacity(n, H, W, K) if capacity is None else int(capacity)
    stream = torch.cuda.current_stream(dev)
    ws = workspace('rle.encode', dev, stream, nbytes)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n * K + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(L.rmem_rle_encode_labels(labels.data_ptr(), n, H, W, K, ws.data_ptr(), out.data_ptr(), cap, offsets.data_ptr(),
                                        status.data_ptr(), stream.cuda_stream), 'rmem_rle_encode_labels')
    labels.record_stream(stream)
    return out[:cap], offsets, status


def encode_label_stack(labels_u8: torch.Tensor, num_ids: int, squeeze_idx: Optional[Sequence[int]] = None, boxes: bool = False,
                       ascii: bool = False) -> List[Dict[int, dict]]:
    """Per frame of a uint8 device label stack [n, H, W] or [H, W]: {object id: {'size': [H, W], 'counts': bytes}} for the ids
    1..num_ids (a mask the frame does not hold is the one-count string of the empty mask).  ascii: counts as str, for json.dump.
    squeeze_idx: the keys are squeeze_idx[id] (save_masks' un-squeeze); ids beyond its length are left out.  boxes: every entry
    also gets 'area' and 'bbox' = [x, y, w, h] from the census (evaluator.object_boxes; [0, 0, 0, 0] for an empty mask).
    Per chunk of frames_per_call frames: one encode call, then fetch_files' two device-to-host copies.  When the default capacity
    was too small (the status word), the chunk is encoded once more with the exact size the offsets reported."""
    labels = uint8_stack(labels_u8, 'rle.encode_label_stack')
    n, H, W = labels.shape
    K = int(num_ids)
    if not 1 <= K <= 255:
        raise _lib.RmemError(f'rle.encode_label_stack: num_ids must be in 1..255 (got {num_ids})')
    stream = torch.cuda.current_stream(labels.device)
    step = frames_per_call(H, W, K)
    strings: List[bytes] = []
    for k in range(0, n, step):
        m = min(step, n - k)
        out, offsets, status = encode(labels[k:k + m], K)
        try:
            strings += fetch_files(out, offsets, m * K, stream, 'rle.encode_label_stack')
        except _lib.RmemError:
            if not int(status.item()) & ST_CAPACITY:
                raise
            out, offsets, status = encode(labels[k:k + m], K, int(offsets[-1].item()))
            strings += fetch_files(out, offsets, m * K, stream, 'rle.encode_label_stack')
    area = box = None
    if boxes:
        from .evaluator import object_boxes
        area, box = (t.cpu().numpy() for t in object_boxes(labels, K))
    keys = object_keys(K, squeeze_idx)
    frames = []
    for f in range(n):
        entry = {}
        for i, key in keys.items():
            s = strings[f * K + i - 1]
            e = {'size': [H, W], 'counts': s.decode('ascii') if ascii else s}
            if boxes:
                a = int(area[f, i - 1])
                x0, y0, x1, y1 = (int(v) for v in box[f, i - 1])
                e['area'], e['bbox'] = a, ([x0, y0, x1 - x0 + 1, y1 - y0 + 1] if a else [0, 0, 0, 0])
            entry[key] = e
        frames.append(entry)
    return frames


# ---------------------------------------------------------------------------------------------------------------- reading

def string_from_counts(counts: Sequence[int]) -> bytes:
    """maskApi.c's rleToString for an uncompressed counts list (pure host code)."""
    out = bytearray()
    counts = [int(c) for c in counts]
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            out.append((c | 0x20 if more else c) + 48)
    return bytes(out)


def _string_of(rle, size, where) -> bytes:
    if not isinstance(rle, dict) or 'counts' not in rle or 'size' not in rle:
        raise _lib.RmemError(f'PackedRles: {where}: an rle is a dict with \'size\' and \'counts\'')
    if tuple(int(v) for v in rle['size']) != size:
        raise _lib.RmemError(f'PackedRles: {where}: size {list(rle["size"])} differs from the stack\'s {list(size)}')
    counts = rle['counts']
    if isinstance(counts, str):
        return counts.encode('latin-1', 'replace')                  # a character beyond a byte becomes '?', which still decodes or fails there
    if isinstance(counts, (bytes, bytearray, memoryview)):
        return bytes(counts)
    return string_from_counts(counts)


class PackedRles(Packed):
    """A clip's masks, packed once: frames[f] is {value: rle} or [(value, rle), ...] (listing order = painting order, the later
    mask wins where two overlap), value the label (1..255) the mask paints, rle = {'size': [H, W], 'counts': bytes, str, or the
    uncompressed list of ints}.  size = (H, W) of the stack; an rle of another size raises here.  The strings sit back to back in
    one pinned buffer, with the descriptor table (RmemRleDesc).  len() is the number of strings; status words are per string."""
    NOUN, STATUS_NAMES = 'RLE string', STATUS_NAMES

    def __init__(self, frames: Sequence, size: Tuple[int, int]):
        self.height, self.width = int(size[0]), int(size[1])
        if len(frames) < 1 or self.height < 1 or self.width < 1 or self.height * self.width > MAX_PIXELS:
            raise _lib.RmemError(f'PackedRles: {len(frames)} frames of {self.height}x{self.width} (at least one frame, H * W at most 2^26)')
        self.shape = torch.Size((len(frames), self.height, self.width))
        strings, self.where = [], []
        for f, entry in enumerate(frames):
            items = list(entry.items()) if isinstance(entry, dict) else list(entry)
            if len(items) > 255:
                raise _lib.RmemError(f'PackedRles: frame {f} lists {len(items)} masks (at most 255)')
            for value, rle in items:
                if not 1 <= int(value) <= 255:
                    raise _lib.RmemError(f'PackedRles: frame {f}: label value {value} outside 1..255')
                strings.append(_string_of(rle, (self.height, self.width), f'frame {f}, value {value}'))
                self.where.append((f, int(value)))
        self.descs = (_lib.RleDesc * max(len(strings), 1))()
        at = 0
        for k, (st, (f, v)) in enumerate(zip(strings, self.where)):
            self.descs[k] = _lib.RleDesc(f, v, at, len(st))
            at += len(st)
        self.nstrings, self.total_bytes = len(strings), at
        host = np.frombuffer(b''.join(strings), dtype=np.uint8).copy() if at else np.zeros(0, dtype=np.uint8)
        self.buf = torch.from_numpy(host)
        self.desc_bytes = torch.frombuffer(bytearray(self.descs), dtype=torch.uint8)
        if torch.cuda.is_available():                                  # packing itself needs no GPU
            self.buf, self.desc_bytes = self.buf.pin_memory(), self.desc_bytes.pin_memory()
        self._dev = {}

    def __len__(self):
        return self.nstrings

    def check(self, device, first: int = 0, count: Optional[int] = None, stream=None):
        """Packed.check, naming the frame and the label value of the first bad string as well"""
        try:
            super().check(device, first, count, stream)
        except _lib.RmemError as e:
            st = self.status(device)[first:first + (len(self) - first if count is None else count)].cpu()
            k = first + int(torch.nonzero(st).flatten()[0])
            raise _lib.RmemError(f'{e} [string {k}: frame {self.where[k][0]}, value {self.where[k][1]}]') from None


def decode_labels_into(packed: PackedRles, out: torch.Tensor, stream=None):
    """Every frame of `packed` into out (uint8 [n, H, W], contiguous, device) on ``stream`` (a torch.cuda.Stream or a raw handle;
    default: the current stream).  Nothing waits for the GPU: the strings are copied from pinned memory on the stream, the status
    words land in packed.status(device) and are read later by packed.check(device).  A pack without any string zero-fills out."""
    if not isinstance(packed, PackedRles):
        raise _lib.RmemError('rle.decode_labels_into: packed must be a PackedRles')
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda:
        raise _lib.RmemError('rle.decode_labels_into: out must be a uint8 device tensor')
    if tuple(out.shape) != tuple(packed.shape) or not out.is_contiguous():
        raise _lib.RmemError(f'rle.decode_labels_into: out must be a contiguous {list(packed.shape)} tensor (got {list(out.shape)})')
    n, H, W = packed.shape
    dev = out.device
    ts = stream_of(dev, stream)
    if packed.nstrings == 0:
        with torch.cuda.stream(ts):
            out.zero_()
        return
    L = _lib.lib()
    nbytes = L.rmem_rle_decode_workspace_bytes(packed.nstrings, packed.total_bytes, n, W)
    if nbytes == 0:
        raise _lib.RmemError(f'rle.decode_labels_into: {packed.nstrings} strings of {packed.total_bytes} bytes for {n} frames: too many')
    dc = packed.on_device(dev)
    ws = workspace('rle.decode', dev, ts, nbytes)
    dc.used_on(ts)
    out.record_stream(ts)
    if packed.total_bytes:
        from . import ops
        ops.copy_async(dc.bits[:packed.total_bytes], packed.buf, packed.total_bytes)(ts.cuda_stream)
    _lib.check(L.rmem_rle_decode_labels(dc.bits.data_ptr(), packed.total_bytes, dc.descs.data_ptr(), packed.nstrings, n, H, W, ws.data_ptr(),
                                        out.data_ptr(), dc.status.data_ptr(), ts.cuda_stream), 'rmem_rle_decode_labels')


def decode_label_stack(frames, size: Optional[Tuple[int, int]] = None, device=None) -> torch.Tensor:
    """uint8 [n, H, W] label maps on `device` of a clip's masks (what PackedRles takes, or a PackedRles): label[mask] = value per
    frame in listing order, 0 under no mask.  One decode call, then one synchronisation and one readback of the status words: a
    non-zero word raises RmemError naming the string and the reasons."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.RmemError('rle.decode_label_stack: the target must be a GPU device (there is no host decoder)')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    packed = frames if isinstance(frames, PackedRles) else PackedRles(frames, size)
    stream = torch.cuda.current_stream(device)
    out = torch.empty(tuple(packed.shape), dtype=torch.uint8, device=device)
    decode_labels_into(packed, out, stream)
    if packed.nstrings:
        packed.check(device, 0, packed.nstrings, stream)
    return out
