"""Exact Euclidean distance transform of label stacks on the device, and what is built on it: the peaks of a distance map per
key value, and the Hausdorff distance of every object of two stacks (include/rmem.h: rmem_label_edt, rmem_label_edt_peaks).

All distances are SQUARED distances between pixel centres as int32: exact, no float anywhere on the device.  2^31 - 1 (SENTINEL)
stands where there is nothing to measure a distance to.  Everything runs on the current stream; the stacks never leave the device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import frames_per_pass, int_in, stack as _frames, stack_pair
from ._lib import RmemError

SENTINEL = 2 ** 31 - 1
MAX_SIDE = 16384                             # csrc/label_edt.hip: kMaxSide


def _geometry(what: str, a: torch.Tensor):
    n, H, W = a.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise RmemError(f'{what}: frames of {H} x {W} are too large (H and W at most {MAX_SIDE})')
    return n, H, W


def _edt(a, value, border, dist2, g, stream):
    n, H, W = a.shape
    _lib.check(_lib.lib().rmem_label_edt(a.data_ptr(), n, H, W, value, border, dist2.data_ptr(), g.data_ptr(), g.numel(), stream.cuda_stream),
               'rmem_label_edt')


def _peaks(dist2, keys, table, ws, stream):
    n, H, W = keys.shape
    _lib.check(_lib.lib().rmem_label_edt_peaks(dist2.data_ptr(), keys.data_ptr(), n, H, W, table.data_ptr(), ws.data_ptr(), ws.numel(),
                                               stream.cuda_stream), 'rmem_label_edt_peaks')


def label_edt(labels_u8: torch.Tensor, value: Optional[int] = None, border: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [n, H, W] on the device ([H, W] for a 2-D input): the squared Euclidean distance of every pixel
      value None   to the nearest pixel of its frame that holds ANOTHER value -- the depth of every object's interior and, on the
                   background, the distance to the nearest object.  border=True: the outside of the frame counts as another value
                   (min(y + 1, H - y, x + 1, W - x)^2 joins the minimum: a frame padded with zeros); False: it counts as nothing;
      value 0..255 to the nearest pixel that holds `value`, 0 on those pixels: scipy's distance_transform_edt(labels != value),
                   squared.  border is ignored (passed as 0).
    SENTINEL where there is no such pixel: a frame of one value without border, a frame that does not hold `value`.  A void label of
    255 is an ordinary value.  labels_u8: uint8 device stack [n, H, W] or [H, W], H and W at most 16384.  out: None allocates; an
    int32 contiguous device tensor of the labels' shape is written.  The vertical distances live in a workspace per (device,
    stream).  Two launches on the current stream, no host sync."""
    what = 'distance.label_edt'
    v = -1 if value is None else int_in(what, 'value', value, 0, 255, 'None or an integer in')
    a = _frames(what, labels_u8)
    n, H, W = _geometry(what, a)
    if out is None:
        dist2 = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    else:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != a.device or out.shape != labels_u8.shape
                or not out.is_contiguous()):
            raise RmemError(f'{what}: out must be a contiguous int32 tensor of the labels\' shape on their device')
        dist2 = out.view(a.shape)
    stream = torch.cuda.current_stream(a.device)
    g = workspace('edt', a.device, stream, int(_lib.lib().rmem_label_edt_workspace_bytes(n, H, W)))
    _edt(a, v, int(bool(border)) if value is None else 0, dist2, g, stream)
    for t in (a, dist2):
        t.record_stream(stream)
    return dist2.view(labels_u8.shape) if out is None else out


def peaks(dist2: torch.Tensor, keys_u8: torch.Tensor) -> torch.Tensor:
    """int32 [n, 256, 2] on the device: for every frame and every value v of keys_u8 (the largest dist2 among the pixels with
    keys == v, the flat index y * W + x of the first such pixel in raster order that attains it); (-1, -1) for a value no pixel of
    the frame holds.  dist2: label_edt's int32 map (not negative); keys_u8: a uint8 device stack of the same shape -- the labels
    themselves (the deepest point of every object) or the other stack of a pair.  Three launches, no host sync."""
    what = 'distance.peaks'
    if isinstance(dist2, torch.Tensor) and isinstance(keys_u8, torch.Tensor) and dist2.shape != keys_u8.shape:
        raise RmemError(f'{what}: dist2 and keys must have one shape (got {tuple(dist2.shape)} and {tuple(keys_u8.shape)})')
    k = _frames(what, keys_u8, 'keys')
    if not isinstance(dist2, torch.Tensor) or dist2.dtype != torch.int32 or dist2.device != k.device:
        raise RmemError(f'{what}: dist2 must be an int32 tensor of the keys\' shape on their device')
    d = dist2.contiguous()
    n = k.shape[0]
    stream = torch.cuda.current_stream(k.device)
    table = torch.empty(n, 256, 2, dtype=torch.int32, device=k.device)
    ws = workspace('edt_peaks', k.device, stream, int(_lib.lib().rmem_label_edt_peaks_workspace_bytes(n)))
    _peaks(d, k, table, ws, stream)
    for t in (d, k):
        t.record_stream(stream)
    return table


def hausdorff2(a_u8: torch.Tensor, b_u8: torch.Tensor, num_objs: int, workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """int32 [n, num_objs] on the device: column i - 1 is the squared Hausdorff distance of the pixel sets A = {a == i} and
    B = {b == i} on every frame, max(max over A of the squared distance to B, max over B of that to A); 0 where both are empty,
    SENTINEL where exactly one is.  The number that shows a far-away false blob which the region similarity barely notices.  A
    void label of 255 is an ordinary value here: its pixels belong to no object 1..num_objs of that stack (and would be object 255
    with num_objs = 255).  a_u8, b_u8: uint8 device stacks of one shape, [n, H, W] or [H, W].  Per object two to-value transforms
    and two peaks keyed by the other stack.  The distance map, the vertical distances and the tables live in a workspace per
    (device, stream) of as many frames as fit workspace_bytes (default: 256 MiB, or one frame's need where that is larger); the
    call walks the stacks that many frames at a time.  No host sync."""
    what = 'distance.hausdorff2'
    K = int_in(what, 'num_objs', num_objs, 1, 255)
    a, b = stack_pair(what, a_u8, b_u8)
    for t in (a, b):
        _frames(what, t)
    n, H, W = _geometry(what, a)
    L = _lib.lib()
    HW4 = H * W * 4
    g1, p1 = int(L.rmem_label_edt_workspace_bytes(1, H, W)), int(L.rmem_label_edt_peaks_workspace_bytes(1))
    per_frame = HW4 + g1 + 2 * p1                                    # the map, g, the keys and one table
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]
    stream = torch.cuda.current_stream(a.device)
    ws = workspace('hausdorff', a.device, stream, k * per_frame)
    keys = ws[:k * p1]                                               # widest alignment first
    table = ws[k * p1:2 * k * p1].view(torch.int32).view(k, 256, 2)
    dmap = ws[2 * k * p1:2 * k * p1 + k * HW4].view(torch.int32)
    g = ws[2 * k * p1 + k * HW4:k * per_frame]
    out = torch.empty(n, K, dtype=torch.int32, device=a.device)
    for f0 in range(0, n, k):
        sa, sb = a[f0:f0 + k], b[f0:f0 + k]
        m = sa.shape[0]
        for i in range(1, K + 1):
            col = out[f0:f0 + m, i - 1]
            _edt(sb, i, 0, dmap, g, stream)                          # to B, read on A
            _peaks(dmap, sa, table, keys, stream)
            col.copy_(table[:m, i, 0])
            _edt(sa, i, 0, dmap, g, stream)                          # to A, read on B
            _peaks(dmap, sb, table, keys, stream)
            torch.maximum(col, table[:m, i, 0], out=col)
    out.clamp_(min=0)                                                # (-1, -1): both sets empty
    for t in (a, b):
        t.record_stream(stream)
    return out


def hausdorff(a_u8: torch.Tensor, b_u8: torch.Tensor, num_objs: int) -> np.ndarray:
    """float64 numpy [n, num_objs]: the Hausdorff distance in pixels of object i = 1..num_objs of two stacks on every frame -- the
    square root of hausdorff2, inf where exactly one of the two sets is empty, 0 where both are.  One readback."""
    h2 = hausdorff2(a_u8, b_u8, num_objs).cpu().numpy()
    return np.where(h2 == SENTINEL, np.inf, np.sqrt(h2.astype(np.float64)))
