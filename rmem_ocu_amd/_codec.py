"""Host plumbing the image codecs (png, jpeg) and the clip scorer (evaluator.clip_counts) share: the palette, streams, the
grow-only device workspaces, the pinned readback of packed files, the check of a label stack, a packed clip's copy on a device.
Device plumbing lives here; the argument checks of the modules on label stacks (pairs, components, polygons, rle) are _labels'."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from ._lib import RmemError

_streams: Dict[Tuple[int, int], torch.cuda.Stream] = {}
_workspaces: Dict[Tuple[str, int, int], torch.Tensor] = {}     # (kind, device index, stream) -> uint8 buffer, grow-only
_pinned: Dict[Tuple[str, int], List[torch.Tensor]] = {}         # (kind, device index) -> [offsets, bytes] pinned host buffers, grow-only


def davis_palette() -> List[int]:
    """The 256-colour DAVIS palette (bit-reversal colour map; the same table utils/image.py:8-62 hard-codes)."""
    pal = []
    for i in range(256):
        r = g = b = 0
        c = i
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal += [r, g, b]
    return pal


def _index(device) -> int:
    return device.index or 0


def stream_of(device, stream=None) -> torch.cuda.Stream:
    """None: the current stream; a torch.cuda.Stream: itself; a raw handle: its (cached) ExternalStream"""
    if stream is None:
        return torch.cuda.current_stream(device)
    if isinstance(stream, torch.cuda.Stream):
        return stream
    key = (_index(device), int(stream))
    st = _streams.get(key)
    if st is None:
        st = _streams[key] = torch.cuda.ExternalStream(int(stream), device=device)
    return st


# Device buffers that only one stream's kernels touch are ALLOCATED ON THE STREAM THAT RUNS THOSE KERNELS: when one is dropped
# (a workspace grown, a pointer table evicted), the caching allocator hands its block back only to later allocations on that
# same stream, which run after the queued kernels that still read or write it.

def workspace(kind: str, device, stream, nbytes: int) -> torch.Tensor:
    """The uint8 scratch buffer of `kind` for ``stream`` (as stream_of takes it): calls on one stream run in order, so they share
    one buffer per kind, which only grows."""
    ts = stream_of(device, stream)
    key = (kind, _index(device), ts.cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        with torch.cuda.stream(ts):
            ws = _workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def split_files(data: bytes, off: List[int], capacity: int, what: str) -> List[bytes]:
    """data[off[i]:off[i + 1]] per file, after checking the offsets a device call wrote: they start at 0, grow strictly and end
    within `capacity`"""
    if off[0] != 0 or off[-1] > capacity or any(b <= a for a, b in zip(off, off[1:])):
        raise RmemError(f'{what}: bad offsets from the device ({off[:4]} ... {off[-1]})')
    return [data[a:b] for a, b in zip(off, off[1:])]


def _pinned_pair(kind: str, device, noffsets: int, nbytes: int) -> List[torch.Tensor]:
    bufs = _pinned.setdefault((kind, _index(device)), [torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.uint8)])
    for i, n in ((0, noffsets), (1, nbytes)):
        if bufs[i].numel() < n:
            bufs[i] = torch.empty(n, dtype=bufs[i].dtype).pin_memory()
    return bufs


def fetch_files(out: torch.Tensor, offsets: torch.Tensor, m: int, stream: torch.cuda.Stream, what: str) -> List[bytes]:
    """The m files an encode call on ``stream`` packed into `out` (file f = out[offsets[f]:offsets[f + 1]]): exactly two
    device-to-host copies into pinned memory -- the offsets, then the offsets[m] bytes -- each followed by a synchronise.
    what: 'module.function' for the error text; the module names the pinned pair, one per codec and device."""
    kind = what.split('.')[0]
    off_h = _pinned_pair(kind, out.device, m + 1, 0)[0]
    off_h[:m + 1].copy_(offsets, non_blocking=True)
    stream.synchronize()
    off = off_h[:m + 1].tolist()
    total = off[m] if 0 < off[m] <= out.numel() else 0          # a bad total: nothing is copied and split_files raises
    data_h = _pinned_pair(kind, out.device, m + 1, total)[1]
    data_h[:total].copy_(out[:total], non_blocking=True)
    stream.synchronize()
    return split_files(data_h[:total].numpy().tobytes(), off, out.numel(), what)


def uint8_stack(t, what: str, name: str = 'labels') -> torch.Tensor:
    """the [n, H, W] view of a non-empty uint8 device stack [n, H, W] or [H, W]; anything else raises"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
        raise RmemError(f'{what}: {name} must be a uint8 device tensor')
    if t.dim() not in (2, 3) or t.numel() == 0:
        raise RmemError(f'{what}: {name} must be a non-empty [n, H, W] or [H, W] stack (got {tuple(t.shape)})')
    return t[None] if t.dim() == 2 else t


class DeviceCopy:
    """A pack on one device: the pack buffer's allocation (filled range by range), the descriptor table and one status word per
    frame."""

    def __init__(self, packed: 'Packed', device):
        self.bits = torch.empty(max(packed.buf.numel(), 1), dtype=torch.uint8, device=device)
        self.descs = packed.desc_bytes.to(device)                      # once per pack and device
        self.status = torch.zeros(len(packed), dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()                # both are complete before any decode stream reads them

    def used_on(self, stream: torch.cuda.Stream):
        """these buffers are read / written on ``stream``: freeing the pack must not hand them out before it catches up"""
        for t in (self.bits, self.descs, self.status):
            t.record_stream(stream)


class Packed:
    """What PackedPngs and PackedJpegs share.  A subclass sets NOUN and STATUS_NAMES (bit -> reason) and, when it is built, buf
    (the pinned pack), desc_bytes, descs and _dev = {} (device index -> DeviceCopy)."""
    NOUN = ''
    STATUS_NAMES: Dict[int, str] = {}

    def __len__(self):
        return len(self.descs)

    def on_device(self, device) -> DeviceCopy:
        device = torch.device(device)
        key = _index(device)
        if key not in self._dev:
            self._dev[key] = DeviceCopy(self, device)
        return self._dev[key]

    def status(self, device) -> torch.Tensor:
        return self.on_device(device).status

    def check(self, device, first: int = 0, count: Optional[int] = None, stream=None):
        """Synchronise ``stream`` (the one the frames were decoded on; default: the current stream) and raise RmemError naming the
        first frame of first .. first+count-1 whose status word is not zero, and its bits."""
        device = torch.device(device)
        count = len(self) - first if count is None else count
        stream_of(device, stream).synchronize()
        st = self.status(device)[first:first + count].cpu()
        bad = torch.nonzero(st).flatten().tolist()
        if bad:
            k = bad[0]
            reasons = ', '.join(v for b, v in self.STATUS_NAMES.items() if int(st[k]) & b)
            raise RmemError(f'{self.NOUN} frame {first + k} failed to decode on the GPU (status {int(st[k])}: {reasons})'
                            + (f'; {len(bad)} frames bad' if len(bad) > 1 else ''))
