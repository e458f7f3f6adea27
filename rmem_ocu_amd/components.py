"""Connected components of label stacks on the device, and the clean-up of predicted masks built on them.

The label census (protocol.label_census) knows the area and the box of every label VALUE; nothing there knows the PIECES of a
value.  label_components gives every pixel the first pixel (in raster order) of its piece, component_stats the area, the
neighbouring values and the border contact of every piece and a per-value summary, clean_labels the usual post-processing of a
segmentation pipeline in one pass -- fill small holes inside an object, drop small specks, keep only the largest piece of every
object -- and object_fragments the number of pieces per frame and object (include/rmem.h, rmem_label_components,
rmem_label_component_stats, rmem_label_clean).  Everything runs on the current stream; the stacks never leave the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._codec import workspace
from ._labels import connectivity as _connectivity, frames_per_pass, int_in, is_int, stack as _frames
from ._lib import RmemError


def tile() -> Tuple[int, int]:
    """(rows, columns) of the tile the first kernel works on: where the seams of a frame lie"""
    th, tw = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().rmem_label_components_tile(C.byref(th), C.byref(tw)), 'rmem_label_components_tile')
    return th.value, tw.value


def _area(what: str, name: str, v) -> int:
    if not is_int(v) or int(v) < 0:
        raise RmemError(f'{what}: {name} must be a non-negative integer (got {v!r})')
    return int(min(int(v), 2 ** 31 - 1))


def _status(what: str, status, device) -> torch.Tensor:
    if (not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.numel() != 1 or not status.is_cuda
            or status.device != device):
        raise RmemError(f'{what}: status must be an int32 tensor of one element on the labels\' device')
    return status


def _components(a, conn, roots, status, stream):
    n, H, W = a.shape
    _lib.check(_lib.lib().rmem_label_components(a.data_ptr(), n, H, W, conn, roots.data_ptr(), status.data_ptr(), stream.cuda_stream),
               'rmem_label_components')


def _stats(a, roots, conn, stats, table, stream):
    n, H, W = a.shape
    _lib.check(_lib.lib().rmem_label_component_stats(a.data_ptr(), roots.data_ptr(), n, H, W, conn, stats.data_ptr(), table.data_ptr(),
                                                     stream.cuda_stream), 'rmem_label_component_stats')


def label_components(labels_u8: torch.Tensor, connectivity: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(roots int32 [n, H, W], status int32 [1]) on the device: roots[f, y, x] is the flat index y' * W + x' of the first pixel in
    raster order of the component of (y, x) -- the pixels of frame f that hold the same value and are linked by a path of such
    pixels under `connectivity` (4: edge neighbours, 8: corner neighbours too).  Every value counts, 0 included: its components
    are the holes and the background; a void label of 255 is an ordinary value (predicted stacks hold none).  The result does not
    depend on scheduling.  status stays 0; a set bit says that a bounded loop of the kernels ran out (a bug, never a condition).
    labels_u8: uint8 device stack [n, H, W] or [H, W].  Three launches on the current stream, no host sync."""
    what = 'components.label_components'
    conn = _connectivity(what, connectivity)
    a = _frames(what, labels_u8)
    stream = torch.cuda.current_stream(a.device)
    roots = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    _components(a, conn, roots, status, stream)
    a.record_stream(stream)
    return roots, status


def component_stats(labels_u8: torch.Tensor, roots: torch.Tensor, connectivity: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(stats int32 [n, H * W, 4], table int32 [n, 256, 3]) on the device, from a stack and label_components' roots of the same
    connectivity.  stats[f, r] at a root's flat index r: (area, nb_min, nb_max, border) -- the pixel count, the smallest and the
    largest value among the in-frame pixels next to the component that hold another value ((256, -1): the component is the whole
    frame), and 1 if the component touches the frame's edge; (0, 256, -1, 0) anywhere else.  table[f, v]: (number of components of
    value v, area of the largest, root of the largest -- the smallest root on equal areas), (0, 0, -1) for an absent value.
    Four launches on the current stream, no host sync."""
    what = 'components.component_stats'
    conn = _connectivity(what, connectivity)
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    if not isinstance(roots, torch.Tensor) or roots.dtype != torch.int32 or roots.device != a.device or roots.numel() != a.numel():
        raise RmemError(f'{what}: roots must be label_components\' int32 tensor for these labels, on their device')
    roots = roots.contiguous()
    stream = torch.cuda.current_stream(a.device)
    stats = torch.empty(n, H * W, 4, dtype=torch.int32, device=a.device)
    table = torch.empty(n, 256, 3, dtype=torch.int32, device=a.device)
    _stats(a, roots, conn, stats, table, stream)
    for t in (a, roots):
        t.record_stream(stream)
    return stats, table


def clean_labels(labels_u8: torch.Tensor, max_hole_area: int = 0, max_sprinkle_area: int = 0, keep_largest: bool = False,
                 connectivity: int = 8, out: Optional[torch.Tensor] = None, workspace_bytes: Optional[int] = None,
                 status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The cleaned stack (uint8, the shape of labels_u8), one pass in which every decision is taken from the INPUT's components, so
    the result does not depend on any order.  A pixel of value v whose component has (area, nb_min, nb_max, border):
      hole     v == 0, area <= max_hole_area, border == 0 and nb_min == nb_max -> nb_min: a hole wholly inside one object is
               filled with it; a hole between two objects, or one that touches the frame's edge, is left alone;
      removed  v != 0 and (area <= max_sprinkle_area, or keep_largest and the component is not the largest of value v -- the one
               with the smallest root among equals) -> nb_min where nb_min == nb_max, else 0: a speck on the background becomes
               background, a speck wholly inside another object becomes that object, one that straddles several background;
      and v otherwise.  Areas of 0 and keep_largest=False are the identity.  A void label of 255 is an ordinary value here: a
    piece of it is a piece like any other, and a neighbour like any other.  Predicted stacks do not hold it.
    labels_u8: uint8 device stack [n, H, W] or [H, W].  out: None allocates, labels_u8 itself cleans in place, any other uint8
    device tensor of the same shape is written.  The roots, statistics and tables live in a workspace per (device, stream) of as
    many frames as fit workspace_bytes (default: 256 MiB, or one frame's need where that is larger); the call walks the stack that
    many frames at a time.  status: None -- one 4-byte readback after the last pass, RmemError if a kernel's bounded loop ran out;
    a caller's int32 [1] device tensor is OR-ed into instead (the caller zeroes it) and the call makes no host sync."""
    what = 'components.clean_labels'
    conn = _connectivity(what, connectivity)
    hole, speck = _area(what, 'max_hole_area', max_hole_area), _area(what, 'max_sprinkle_area', max_sprinkle_area)
    if out is not None and (not isinstance(out, torch.Tensor) or not isinstance(labels_u8, torch.Tensor) or out.shape != labels_u8.shape):
        raise RmemError(f'{what}: out must be a tensor of the labels\' shape (got {tuple(getattr(out, "shape", ()))} for '
                        f'{tuple(getattr(labels_u8, "shape", ()))})')
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    if out is None:
        dst = torch.empty_like(a)
    else:
        if out.dtype != torch.uint8 or out.device != a.device or not out.is_contiguous():
            raise RmemError(f'{what}: out must be a contiguous uint8 tensor on the labels\' device')
        if out.data_ptr() == labels_u8.data_ptr() and not labels_u8.is_contiguous():
            raise RmemError(f'{what}: cleaning in place needs a contiguous stack')
        dst = out.view(a.shape)
    L = _lib.lib()
    per_frame = int(L.rmem_label_components_workspace_bytes(1, H, W))
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]
    stream = torch.cuda.current_stream(a.device)
    own_status = status is None
    st = torch.zeros(1, dtype=torch.int32, device=a.device) if own_status else _status(what, status, a.device)
    ws = workspace('components', a.device, stream, k * per_frame)
    HW = H * W
    stats = ws[:k * HW * 16].view(torch.int32)                     # the 16-byte entries first: the buffer's own alignment
    roots = ws[k * HW * 16:k * HW * 20].view(torch.int32)
    table = ws[k * HW * 20:k * per_frame].view(torch.int32)
    for f0 in range(0, n, k):
        src, d = a[f0:f0 + k], dst[f0:f0 + k]
        m = src.shape[0]
        _components(src, conn, roots, st, stream)
        _stats(src, roots, conn, stats, table, stream)
        _lib.check(L.rmem_label_clean(src.data_ptr(), d.data_ptr(), roots.data_ptr(), stats.data_ptr(), table.data_ptr(), m, H, W,
                                      hole, speck, int(bool(keep_largest)), stream.cuda_stream), 'rmem_label_clean')
    for t in (a, dst, st):
        t.record_stream(stream)
    if own_status:
        bits = int(st.item())
        if bits:
            raise RmemError(f'{what}: a bounded loop of the component kernels ran out (status {bits}: '
                            f'{", ".join(s for b, s in ((1, "union"), (2, "find")) if bits & b)}); this is a bug')
    return dst.view(labels_u8.shape) if out is None else out


def object_fragments(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8) -> torch.Tensor:
    """int32 [n, num_objs + 1] on the device: the number of pieces of every value 0..num_objs on every frame (column 0 of
    component_stats' table; column 0 here is the background's pieces).  1 everywhere for a clean prediction; a 3 says that the
    object's mask fell into three parts on that frame.  No host sync."""
    K = int_in('components.object_fragments', 'num_objs', num_objs, 1, 255)
    roots, _ = label_components(labels_u8, connectivity)
    _, table = component_stats(labels_u8, roots, connectivity)
    return table[:, :K + 1, 0].contiguous()
