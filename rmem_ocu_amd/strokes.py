"""Strokes drawn into uint8 label stacks on the device: scribbles, clicks and polylines with a round brush or as hairlines.

The interactive side of a VOS engine speaks in strokes: evaluator.next_clicks and next_scribbles produce them from an error map,
labelling tools (CVAT's polylines and points) and DAVIS-interactive scribble files store them, and evaluator.labels_from_seeds
turns a sparse seed stack into a full label map.  This module turns the strokes into that stack without a host rasteriser and
without the upload of H * W bytes per frame (include/rmem.h, rmem_stroke_draw_labels, has the contract: pixel-INDEX coordinates,
the centre of pixel (y, x) at (x, y), exact on 1/256-pixel fixed point; a round brush covers the pixel centres within r of the
polyline, r = 0 is an 8-connected digital line that draws a path of 8-neighbour pixels back onto itself; the later stroke of a
frame wins, value 0 erases).  PackedStrokes quantises and cuts a clip's strokes on the host; only their segments cross to the
device.  Not the DAVIS toolkit's Bresenham and Bezier code: pixels can differ from it.

    seeds = strokes.draw_label_stack(frames, (H, W), device)                    # frames[f] = [{'value', 'path', 'radius'}, ...]
    strokes.draw_labels_into(packed, labels, over=True)                         # over an existing stack, no host sync
    seeds = evaluator.seeds_from_scribbles(evaluator.next_scribbles(pred, gt, k), (H, W), device)
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import Packed, stream_of, workspace
from ._labels import MAX_FRAMES, MAX_PIXELS, WORKSPACE_CAP, is_int
from ._lib import RmemError

ST_DESC, ST_PREFIX, ST_SEGMENT = 1, 2, 4     # include/rmem.h
STATUS_NAMES = {ST_DESC: 'bad stroke table entry, or a segment of a stroke outside the pass',
                ST_PREFIX: 'the work-item prefix disagrees with a segment',
                ST_SEGMENT: 'a segment coordinate out of range, a hairline segment against its major axis or a segment outside the stroke\'s box'}
FIXED = 256                                  # fixed-point steps per pixel
MAX_COORD = 2 ** 20                          # |x|, |y| of a point, in pixels
MAX_RADIUS = 256                             # pixels
MAX_ITEMS = 2 ** 31 - 1
STROKE_DTYPE = np.dtype([(k, '<i4') for k in ('frame', 'value', 'radius', 'x0', 'y0', 'x1', 'y1', 'slot')])   # RmemStroke


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _path(p, where: str) -> np.ndarray:
    """float64 [k, 2], k >= 1, of a path given as [k, 2] or flat"""
    try:
        a = np.asarray(p, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is not None and a.ndim == 1:
        if a.size % 2:
            raise RmemError(f'PackedStrokes: {where}: a flat path of {a.size} numbers (x0, y0, x1, y1, ...: an even count)')
        a = a.reshape(-1, 2)
    if a is None or a.ndim != 2 or a.shape[1] != 2:
        raise RmemError(f'PackedStrokes: {where}: a path is an array-like [k, 2] of (x, y) or a flat sequence x0, y0, x1, y1, ...')
    if a.shape[0] < 1:
        raise RmemError(f'PackedStrokes: {where}: a path without a point (at least 1)')
    return a


def _stroke(item, where: str) -> Tuple[int, np.ndarray, float]:
    """(value, path, radius) of a stroke in either form PackedStrokes takes"""
    if isinstance(item, dict):
        if 'value' not in item or 'path' not in item:
            raise RmemError(f'PackedStrokes: {where}: a stroke dict has \'value\', \'path\' and an optional \'radius\'')
        value, path, radius = item['value'], item['path'], item.get('radius', 0)
    elif isinstance(item, (tuple, list)) and len(item) in (2, 3):
        value, path, radius = item[0], item[1], (item[2] if len(item) == 3 else 0)
    else:
        raise RmemError(f'PackedStrokes: {where}: a stroke is a dict with \'value\', \'path\' and an optional \'radius\', or a '
                        f'(value, path, radius) tuple')
    if not _is_number(value) or int(value) != value or not 0 <= int(value) <= 255:
        raise RmemError(f'PackedStrokes: {where}: value {value!r} outside 0..255')
    if not _is_number(radius) or not 0 <= float(radius) <= MAX_RADIUS:          # NaN fails both comparisons
        raise RmemError(f'PackedStrokes: {where}: radius must be a finite number in 0..{MAX_RADIUS} pixels (got {radius!r})')
    return int(value), _path(path, where), float(radius)


class PackedStrokes(Packed):
    """A clip's strokes, packed once: frames[f] is a list of strokes in painting order (the later stroke wins where two overlap;
    a frame may list none).  A stroke is {'value': 0..255, 'path': points, 'radius': r} -- 'radius' optional, 0 when absent -- or a
    (value, path, radius) tuple; value 0 erases.  A path is an array-like [k, 2] of (x, y) or a flat sequence x0, y0, x1, y1, ...,
    k >= 1; one point is a click.  origin='centre' (the default): pixel-INDEX coordinates, the centre of pixel (y, x) at (x, y), as
    evaluator.next_clicks, next_scribbles and the DAVIS toolkit have them; origin='corner': the polygon fill's convention, pixel
    corners at integers -- one half is subtracted.  radius r in 0..256 pixels: a round brush that covers the pixel centres within r
    of the polyline; 0 (after rounding to 1/256) is a hairline, an 8-connected digital line.  size = (H, W) of the stack.
    Packing needs no GPU and is vectorised over the clip: it quantises the points to 1/256 pixel (numpy.rint, ties to even), drops
    consecutive repeated points (a lone point stays), cuts the paths into segments, orients the hairline ones along their major
    axis, computes every segment's box clipped to the frame and its work items (the rows of the box for a round brush; the major
    samples inside the frame plus two for a hairline), drops the segments without any, and builds the prefix of the counts.  One
    pinned int32 buffer holds seg_xy [S, 4], seg_stroke [S], seg_first [S + 1], frame_stroke [n + 1] and the stroked frames; the
    stroke table (RmemStroke) is the descriptor table.  len() is the number of strokes; status words are per stroke."""
    NOUN, STATUS_NAMES = 'stroke', STATUS_NAMES

    def __init__(self, frames: Sequence, size: Tuple[int, int], origin: str = 'centre'):
        self.height, self.width = H, W = int(size[0]), int(size[1])
        n = len(frames)
        if n < 1 or n > MAX_FRAMES or H < 1 or W < 1 or H * W > MAX_PIXELS:
            raise RmemError(f'PackedStrokes: {n} frames of {H}x{W} (at least one frame, at most 65535, H * W at most 2^26)')
        if origin not in ('centre', 'corner'):
            raise RmemError(f'PackedStrokes: origin must be \'centre\' or \'corner\' (got {origin!r})')
        self.shape = torch.Size((n, H, W))
        self.where: List[Tuple[int, int]] = []
        paths: List[np.ndarray] = []
        radii: List[float] = []
        for f, entry in enumerate(frames):
            if isinstance(entry, dict) or not isinstance(entry, (list, tuple)):
                raise RmemError(f'PackedStrokes: frame {f} must be a list of strokes (got {type(entry).__name__})')
            for k, item in enumerate(entry):
                value, path, radius = _stroke(item, f'frame {f}, stroke {k}')
                paths.append(path)
                radii.append(radius)
                self.where.append((f, value))
        S = self.nstrokes = len(self.where)
        lens = np.array([len(p) for p in paths], dtype=np.int64)
        V = np.concatenate(paths) if paths else np.zeros((0, 2), dtype=np.float64)
        if origin == 'corner':
            V = V - 0.5
        of_vertex = np.repeat(np.arange(S, dtype=np.int64), lens)
        bad = np.flatnonzero(~(np.abs(V) <= MAX_COORD).all(axis=1))            # also every NaN and infinity
        if bad.size:
            f, v = self.where[int(of_vertex[bad[0]])]
            x, y = V[bad[0]]
            raise RmemError(f'PackedStrokes: frame {f}, value {v}: point ({x}, {y}) is not finite or beyond 2^20 pixels')
        Q = np.rint(V * FIXED).astype(np.int64)
        first = np.ones(len(Q), dtype=bool)                                    # consecutive repeats leave, a lone point stays
        if len(Q) > 1:
            first[1:] = of_vertex[1:] != of_vertex[:-1]
            keep = first.copy()
            keep[1:] |= (Q[1:] != Q[:-1]).any(axis=1)
            Q, of_vertex = Q[keep], of_vertex[keep]
        count = np.bincount(of_vertex, minlength=S)                            # points per stroke, at least 1
        last = np.ones(len(Q), dtype=bool)
        if len(Q) > 1:
            last[:-1] = of_vertex[1:] != of_vertex[:-1]
        lone = count[of_vertex] == 1
        start = np.flatnonzero(~last | lone)                                   # a point starts a segment to the next; a lone one to itself
        end = np.where(lone[start], start, start + 1)
        seg_stroke = of_vertex[start]
        R = np.rint(np.array(radii, dtype=np.float64) * FIXED).astype(np.int64)
        A, B, Rs = Q[start], Q[end], R[seg_stroke]
        hair = Rs == 0
        d = B - A
        xmajor = np.abs(d[:, 0]) >= np.abs(d[:, 1])
        dM = np.where(xmajor, d[:, 0], d[:, 1])
        flip = hair & (dM < 0)                                                 # a hairline runs up its major axis
        A[flip], B[flip] = B[flip], A[flip].copy()
        lo, hi = np.minimum(A, B), np.maximum(A, B)
        below, above = np.where(hair, 128, 255 - Rs)[:, None], np.where(hair, 128, Rs)[:, None]
        top = np.array([W, H], dtype=np.int64)
        b0 = np.clip((lo + below) >> 8, 0, top)                                # [segments, (x, y)]
        b1 = np.clip(((hi + above) >> 8) + 1, 0, top)
        full = (b0 < b1).all(axis=1)
        am, bm = np.where(xmajor, A[:, 0], A[:, 1]), np.where(xmajor, B[:, 0], B[:, 1])
        ka, kb = np.maximum(0, (am + 255) >> 8), np.minimum(np.where(xmajor, W, H) - 1, bm >> 8)
        samples = np.where((d != 0).any(axis=1), np.maximum(0, kb - ka + 1), 0)
        items = np.where(full, np.where(hair, 2 + samples, b1[:, 1] - b0[:, 1]), 0)
        keep = items > 0
        A, B, b0, b1, seg_stroke, items = A[keep], B[keep], b0[keep], b1[keep], seg_stroke[keep], items[keep]
        E = self.nsegs = int(keep.sum())
        prefix = np.concatenate([[0], np.cumsum(items)])
        self.items = int(prefix[-1])
        if self.items > MAX_ITEMS:
            raise RmemError(f'PackedStrokes: the segments have {self.items} work items (at most 2^31 - 1); pack fewer frames')
        self.seg_xy = np.concatenate([A, B], axis=1).astype(np.int32)
        self.seg_stroke = seg_stroke.astype(np.int32)
        self.seg_first = prefix.astype(np.int32)
        table = np.zeros(S, dtype=STROKE_DTYPE)
        table['frame'], table['value'], table['radius'] = [w[0] for w in self.where], [w[1] for w in self.where], R
        self.stroke_seg = np.searchsorted(seg_stroke, np.arange(S + 1), side='left').astype(np.int64)      # the first segment of every stroke
        held = np.flatnonzero(np.diff(self.stroke_seg))
        if held.size:                                                          # the union of the boxes of a stroke's segments
            at = self.stroke_seg[held]
            table['x0'][held], table['y0'][held] = np.minimum.reduceat(b0[:, 0], at), np.minimum.reduceat(b0[:, 1], at)
            table['x1'][held], table['y1'][held] = np.maximum.reduceat(b1[:, 0], at), np.maximum.reduceat(b1[:, 1], at)
        self.frame_stroke = np.searchsorted(table['frame'], np.arange(n + 1), side='left').astype(np.int32)
        self.stroked = np.flatnonzero(np.diff(self.frame_stroke)).astype(np.int32)                          # the frames that list a stroke
        table['slot'] = np.searchsorted(self.stroked, table['frame'])
        self.table = table
        ns = len(self.stroked)
        self.offsets = (0, 16 * E, 20 * E, 24 * E + 4, 24 * E + 4 + 4 * (n + 1))   # bytes: seg_xy, seg_stroke, seg_first, frame_stroke, stroked
        blob = np.concatenate([self.seg_xy.reshape(-1), self.seg_stroke, self.seg_first, self.frame_stroke, self.stroked]).astype(np.int32)
        assert blob.size == 6 * E + 1 + n + 1 + ns
        self.buf = torch.from_numpy(blob.view(np.uint8))
        self.descs = table
        self.desc_bytes = torch.from_numpy(table.view(np.uint8).reshape(-1).copy() if S else np.zeros(STROKE_DTYPE.itemsize, dtype=np.uint8))
        if torch.cuda.is_available():                                          # packing itself needs no GPU
            self.buf, self.desc_bytes = self.buf.pin_memory(), self.desc_bytes.pin_memory()
        self._dev = {}

    def __len__(self):
        return self.nstrokes

    def passes(self, workspace_bytes: Optional[int] = None) -> List[_lib.StrokePass]:
        """The passes of whole frames draw_labels_into makes: as many consecutive frames each as keep
        rmem_stroke_workspace_bytes of their stroked frames' owner maps at or below workspace_bytes (default:
        _labels.WORKSPACE_CAP, or one frame's need where that is larger); a budget below one frame's need is refused."""
        n, H, W = self.shape
        need = lambda slots: int(_lib.lib().rmem_stroke_workspace_bytes(slots, H, W))
        one = need(1)
        if workspace_bytes is None:
            workspace_bytes = max(one, min(need(max(len(self.stroked), 1)), WORKSPACE_CAP))
        elif not is_int(workspace_bytes) or workspace_bytes < one:
            raise RmemError(f'strokes.draw_labels_into: workspace_bytes must be an integer of at least one frame\'s need, '
                            f'{one} bytes (got {workspace_bytes!r})')
        fs, out, f0 = self.frame_stroke, [], 0
        has = np.diff(fs) > 0
        while f0 < n:
            f1, slots = f0 + 1, int(has[f0])
            while f1 < n and need(slots + int(has[f1])) <= workspace_bytes:
                slots += int(has[f1])
                f1 += 1
            s0, s1 = int(fs[f0]), int(fs[f1])
            e0, e1 = int(self.stroke_seg[s0]), int(self.stroke_seg[s1])
            i0, i1 = int(self.seg_first[e0]), int(self.seg_first[e1])
            slot0 = int(np.searchsorted(self.stroked, f0))
            out.append(_lib.StrokePass(f0, f1 - f0, s0, s1 - s0, e0, e1 - e0, slot0, slots, i0, i1 - i0))
            f0 = f1
        return out

    def check(self, device, first: int = 0, count: Optional[int] = None, stream=None):
        """Packed.check, naming the frame and the value of the first bad stroke as well"""
        try:
            super().check(device, first, count, stream)
        except RmemError as e:
            st = self.status(device)[first:first + (len(self) - first if count is None else count)].cpu()
            k = first + int(torch.nonzero(st).flatten()[0])
            raise RmemError(f'{e} [stroke {k}: frame {self.where[k][0]}, value {self.where[k][1]}]') from None


def draw_pass(packed: PackedStrokes, dc, p: _lib.StrokePass, ws: torch.Tensor, out: torch.Tensor, over: bool, raw_stream: int):
    """one call of rmem_stroke_draw_labels: pass p of `packed`, whose buffers on the device are dc, into out on a raw stream"""
    import ctypes
    n, H, W = packed.shape
    base = dc.bits.data_ptr()
    xy, stroke, first, frames, stroked = (base + o for o in packed.offsets)
    _lib.check(_lib.lib().rmem_stroke_draw_labels(xy, stroke, first, packed.nsegs, dc.descs.data_ptr(), packed.nstrokes, frames, stroked,
                                                  len(packed.stroked), n, H, W, ctypes.byref(p), ws.data_ptr(), ws.numel(), out.data_ptr(),
                                                  int(bool(over)), dc.status.data_ptr(), raw_stream), 'rmem_stroke_draw_labels')


def draw_labels_into(packed: PackedStrokes, out: torch.Tensor, over: bool = False, stream=None, workspace_bytes: Optional[int] = None):
    """Every frame of `packed` into out (uint8 [n, H, W], contiguous, device) on ``stream`` (a torch.cuda.Stream or a raw handle;
    default: the current stream).  over=False: a fresh stack, every byte of out is written, 0 under no stroke.  over=True: only
    the covered bytes change, frames without strokes are not touched.  Nothing waits for the GPU: the pack is copied from pinned
    memory on the stream, the status words land in packed.status(device) and are read later by packed.check(device).  The frames
    go in passes of whole frames whose owner maps (int32 [H, W] per stroked frame) fit workspace_bytes (PackedStrokes.passes: 256
    MiB by default, or one frame's need); a smaller budget is refused.  A pack without any stroke zero-fills a fresh out."""
    what = 'strokes.draw_labels_into'
    if not isinstance(packed, PackedStrokes):
        raise RmemError(f'{what}: packed must be a PackedStrokes')
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda:
        raise RmemError(f'{what}: out must be a uint8 device tensor')
    if tuple(out.shape) != tuple(packed.shape) or not out.is_contiguous():
        raise RmemError(f'{what}: out must be a contiguous {list(packed.shape)} tensor (got {list(out.shape)})')
    plan = packed.passes(workspace_bytes)
    dev = out.device
    ts = stream_of(dev, stream)
    if packed.nstrokes == 0:
        if not over:
            with torch.cuda.stream(ts):
                out.zero_()
        return
    n, H, W = packed.shape
    dc = packed.on_device(dev)
    ws = workspace('strokes', dev, ts, max(int(_lib.lib().rmem_stroke_workspace_bytes(p.slots, H, W)) for p in plan))
    dc.used_on(ts)
    out.record_stream(ts)
    from . import ops
    ops.copy_async(dc.bits[:packed.buf.numel()], packed.buf, packed.buf.numel())(ts.cuda_stream)
    for p in plan:
        draw_pass(packed, dc, p, ws, out, over, ts.cuda_stream)


def draw_label_stack(frames, size: Optional[Tuple[int, int]] = None, device=None, base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [n, H, W] label maps on `device` of a clip's strokes (what PackedStrokes takes, or a PackedStrokes): per frame the
    strokes in listing order, 0 under no stroke -- or, with base (uint8 [n, H, W] on the device), a copy of base drawn over, which
    keeps every byte no stroke covers.  One draw, then one synchronisation and one readback of the status words: a non-zero word
    raises RmemError naming the stroke and the reasons."""
    what = 'strokes.draw_label_stack'
    device = torch.device(device)
    if device.type != 'cuda':
        raise RmemError(f'{what}: the target must be a GPU device (there is no host rasteriser)')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    packed = frames if isinstance(frames, PackedStrokes) else PackedStrokes(frames, size)
    if base is not None and (not isinstance(base, torch.Tensor) or base.dtype != torch.uint8 or base.device != device
                             or tuple(base.shape) != tuple(packed.shape)):
        raise RmemError(f'{what}: base must be a uint8 {list(packed.shape)} tensor on {device}')
    stream = torch.cuda.current_stream(device)
    out = torch.empty(tuple(packed.shape), dtype=torch.uint8, device=device) if base is None else base.clone(memory_format=torch.contiguous_format)
    draw_labels_into(packed, out, base is not None, stream)
    if packed.nstrokes:
        packed.check(device, 0, packed.nstrokes, stream)
    return out
