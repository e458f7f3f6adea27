"""Label stacks thinned to skeletons on the device (Guo and Hall 1989, algorithm A1: the rule of bwmorph's 'thin'), the list of a
stack's non-zero pixels, and the longest path through a skeleton component (include/rmem.h: rmem_label_thin,
rmem_label_pixels_count, rmem_label_pixels_write).

Every value of a stack is thinned as if it were alone in its frame, all of them in one pass; a void label of 255 is an ordinary
value.  The device result is bit-identical to the host restatement of the rule.  Everything runs on the current stream; only the
loss counters (8 bytes per frame) and, in pixels, the totals cross to the host.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import frames_per_pass, is_int, like_labels, stack as _frames
from ._lib import RmemError

# (dy, dx) of the neighbours x1..x8: E, NE, N, NW, W, SW, S, SE (y grows downward)
NEIGHBOURS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


def tile() -> Tuple[int, int, int]:
    """(th, tw, k): the core tile of a thinning launch and the sub-iterations one launch runs (the halo)"""
    th, tw, k = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().rmem_label_thin_tile(C.byref(th), C.byref(tw), C.byref(k)), 'rmem_label_thin_tile')
    return th.value, tw.value, k.value


def table(parity: int) -> np.ndarray:
    """numpy bool [256]: table(parity)[mask] = a pixel whose neighbours x1..x8 are the bits 0..7 of mask is deleted in a
    sub-iteration of that parity (0: even, 1: odd); the constant the kernels use"""
    if not is_int(parity) or int(parity) not in (0, 1):
        raise RmemError(f'skeleton.table: parity must be 0 or 1 (got {parity!r})')
    buf = (C.c_ubyte * 32)()
    _lib.check(_lib.lib().rmem_label_thin_table(int(parity), buf), 'rmem_label_thin_table')
    return np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder='little').astype(bool)


def _thin(src, dst, first, count, lost, ws, stream):
    n, H, W = src.shape
    _lib.check(_lib.lib().rmem_label_thin(src.data_ptr(), n, H, W, first, count, dst.data_ptr(), lost.data_ptr(), ws.data_ptr(), ws.numel(),
                                          stream.cuda_stream), 'rmem_label_thin')


def thin(labels_u8: torch.Tensor, max_iterations: Optional[int] = None, batch: int = 64, out: Optional[torch.Tensor] = None,
         workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """uint8 stack like labels_u8 ([n, H, W] or [H, W], device): every value's skeleton.  An iteration is an even sub-iteration
    followed by an odd one; the skeleton is the state after the first iteration that deletes nothing.
      max_iterations k   exactly k iterations: one call of 2k sub-iterations per pass, no host sync.
      max_iterations None  calls of `batch` sub-iterations (even, at least 2), each continuing in place on the output, until no
                         frame lost a pixel in a call's last two sub-iterations; one readback of 8 bytes per frame per call.  A call
                         that reports a loss removed at least one pixel, so the loop ends.
    out: None allocates; a contiguous uint8 device tensor of the labels' shape is written (it may be labels_u8 itself).  The
    second stack of the rounds lives in a workspace per (device, stream) of as many frames as fit workspace_bytes (default: 256
    MiB, or one frame's need where that is larger); a longer stack goes through in passes of that many frames."""
    what = 'skeleton.thin'
    if max_iterations is not None and (not is_int(max_iterations) or not 0 <= int(max_iterations) <= 2 ** 29):
        raise RmemError(f'{what}: max_iterations must be None or an integer in 0..2^29 (got {max_iterations!r})')
    if not is_int(batch) or int(batch) < 2 or int(batch) % 2 or int(batch) > 2 ** 20:
        raise RmemError(f'{what}: batch must be an even integer in 2..2^20 (got {batch!r})')
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    if out is None:
        res = torch.empty_like(a)
    else:
        res = like_labels(what, out, 'out', torch.uint8, labels_u8, a)
    L = _lib.lib()
    per_frame = int(L.rmem_label_thin_workspace_bytes(1, H, W))
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]
    stream = torch.cuda.current_stream(a.device)
    ws = workspace('thin', a.device, stream, k * per_frame)
    lost = torch.empty(k, 2, dtype=torch.int32, device=a.device)
    for f0 in range(0, n, k):
        src, dst = a[f0:f0 + k], res[f0:f0 + k]
        if max_iterations is not None:
            if max_iterations == 0:
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
            else:
                _thin(src, dst, 0, 2 * int(max_iterations), lost, ws, stream)
            continue
        first = 0
        while True:
            _thin(src, dst, first, int(batch), lost, ws, stream)
            if not lost[:src.shape[0]].cpu()[:, 1].any():                   # the one readback of the call
                break
            src, first = dst, first + int(batch)
    for t in (a, res):
        t.record_stream(stream)
    return res.view(labels_u8.shape) if out is None else out


def pixels(stack_u8: torch.Tensor, samples: Optional[torch.Tensor] = None):
    """(entries int32 [K, 4], totals int32 [n]) on the device: the non-zero pixels of a uint8 device stack ([n, H, W] or [H, W]) as
    rows (frame, y, x, value) in raster order frame by frame, and how many every frame holds.  samples: an int32 device tensor of
    the stack's shape adds a third result, sampled int32 [K] = samples at every listed pixel -- a skeleton pixel's depth from
    distance.label_edt.  Count, one readback of totals (4 bytes per frame), write."""
    what = 'skeleton.pixels'
    a = _frames(what, stack_u8, 'stack')
    n, H, W = a.shape
    if samples is not None and (not isinstance(samples, torch.Tensor) or samples.dtype != torch.int32 or samples.device != a.device
                                or samples.shape != stack_u8.shape):
        raise RmemError(f'{what}: samples must be an int32 tensor of the stack\'s shape on its device')
    L = _lib.lib()
    stream = torch.cuda.current_stream(a.device)
    ws = workspace('pixels', a.device, stream, int(L.rmem_label_pixels_workspace_bytes(n, H, W)))
    totals = torch.empty(n, dtype=torch.int32, device=a.device)
    _lib.check(L.rmem_label_pixels_count(a.data_ptr(), n, H, W, totals.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream),
               'rmem_label_pixels_count')
    K = int(totals.cpu().sum(dtype=torch.int64))
    entries = torch.empty(K, 4, dtype=torch.int32, device=a.device)
    s = None if samples is None else samples.contiguous()
    sampled = None if samples is None else torch.empty(K, dtype=torch.int32, device=a.device)
    if K:
        _lib.check(L.rmem_label_pixels_write(a.data_ptr(), None if s is None else s.data_ptr(), n, H, W, K, entries.data_ptr(),
                                             None if s is None else sampled.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream),
                   'rmem_label_pixels_write')
    for t in (a,) if s is None else (a, s):
        t.record_stream(stream)
    return (entries, totals) if samples is None else (entries, totals, sampled)


def _bfs(yx: np.ndarray, start: int):
    """hops from row `start` and the row that first discovered each row of yx (-1: none); FIFO, neighbours in NEIGHBOURS' order"""
    index = {(int(y), int(x)): i for i, (y, x) in enumerate(yx)}
    dist = np.full(len(yx), -1, dtype=np.int64)
    parent = np.full(len(yx), -1, dtype=np.int64)
    dist[start] = 0
    queue = deque([start])
    while queue:
        i = queue.popleft()
        y, x = int(yx[i, 0]), int(yx[i, 1])
        for dy, dx in NEIGHBOURS:
            j = index.get((y + dy, x + dx))
            if j is not None and dist[j] < 0:
                dist[j], parent[j] = dist[i] + 1, i
                queue.append(j)
    return dist, parent


def component(yx, start: int) -> np.ndarray:
    """the indices of the rows of yx ((y, x) pixels in raster order) that are 8-connected to row `start`, ascending"""
    yx = np.asarray(yx, dtype=np.int64).reshape(-1, 2)
    return np.nonzero(_bfs(yx, int(start))[0] >= 0)[0]


def longest_path(yx) -> np.ndarray:
    """int32 [k, 2]: a long path through one 8-connected skeleton component.  yx: its pixels (y, x) in raster order.  Breadth-first
    search with a FIFO queue, neighbours visited in the order E, NE, N, NW, W, SW, S, SE, distance in hops, a pixel's parent the
    pixel that first discovered it; far(s) is the pixel farthest from s, the smallest raster index among equals.  a = far(first
    pixel), b = far(a); the result is the parent chain from a to b.  On a tree this is a diameter; on a component with loops it is a
    long path, and these steps are its specification.  Host only."""
    yx = np.asarray(yx)
    if yx.ndim != 2 or yx.shape[1] != 2 or yx.shape[0] == 0:
        raise RmemError(f'skeleton.longest_path: yx must be a non-empty [k, 2] array of (y, x) (got shape {yx.shape})')
    yx = yx.astype(np.int64)
    a = int(np.argmax(_bfs(yx, 0)[0]))
    dist, parent = _bfs(yx, a)
    i = int(np.argmax(dist))
    chain = [i]
    while parent[i] >= 0:
        i = int(parent[i])
        chain.append(i)
    return yx[chain[::-1]].astype(np.int32)
