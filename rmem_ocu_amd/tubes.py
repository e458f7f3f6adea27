"""Label pieces through time on the device: tubes, lineage, events, the tube table and the clean-up of flicker.

components.py knows the pieces of every value on ONE frame.  This module joins them over consecutive frames: two pieces of one
value on frames f and f + 1 are linked when they share a pixel (temporal=1) or hold two pixels at most one apart in y and in x
(temporal=9), and a tube is a connected set of pieces under links -- the space-time pieces of a video's labels.  label_tubes gives
every voxel the first voxel of its tube, lineage the predecessors and successors of every piece, piece_events the births, ends,
splits and merges per frame and value, tube_table one row per tube, and clean_tubes removes tubes that live for a few frames only
(include/rmem.h, rmem_label_tubes ... rmem_label_tube_clean).  Tubes cross any boundary a pass would draw, so every function
here takes the stack WHOLE (n * H * W at most 2^31 - 1, 28 bytes of workspace per voxel); nothing walks it in passes.  Everything
runs on the current stream; the stacks never leave the device.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._labels import connectivity as _connectivity, is_int, stack as _frames
from ._lib import RmemError
from .components import _components, _stats, _status

MAX_VOXELS = 2 ** 31 - 1                         # csrc/label_tubes.hip: a voxel's global index is an int


def _temporal(what: str, v) -> int:
    if not is_int(v) or int(v) not in (1, 9):
        raise RmemError(f'{what}: temporal must be 1 or 9 (got {v!r})')
    return int(v)


def _count(what: str, name: str, v) -> int:
    if not is_int(v) or int(v) < 0:
        raise RmemError(f'{what}: {name} must be a non-negative integer (got {v!r})')
    return int(min(int(v), 2 ** 31 - 1))


def _whole(what: str, labels_u8) -> torch.Tensor:
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    if n * H * W > MAX_VOXELS:
        raise RmemError(f'{what}: labels of {n} x {H} x {W} are too large (the stack is taken whole: n * H * W at most 2^31 - 1)')
    return a


def _args(what: str, labels_u8, connectivity, temporal):
    conn, temp = _connectivity(what, connectivity), _temporal(what, temporal)
    a = _whole(what, labels_u8)
    return a, conn, temp, torch.cuda.current_stream(a.device)


def _roots(a, conn, status, stream) -> torch.Tensor:
    roots = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    _components(a, conn, roots, status, stream)
    return roots


def _tubes(a, roots, temp, status, stream) -> torch.Tensor:
    n, H, W = a.shape
    tubes = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    _lib.check(_lib.lib().rmem_label_tubes(a.data_ptr(), roots.data_ptr(), n, H, W, temp, tubes.data_ptr(), status.data_ptr(),
                                           stream.cuda_stream), 'rmem_label_tubes')
    return tubes


def _links(a, roots, temp, stream) -> torch.Tensor:
    n, H, W = a.shape
    links = torch.empty(n, H * W, 4, dtype=torch.int32, device=a.device)
    _lib.check(_lib.lib().rmem_label_tube_lineage(a.data_ptr(), roots.data_ptr(), n, H, W, temp, links.data_ptr(), stream.cuda_stream),
               'rmem_label_tube_lineage')
    return links


def _index(a, tubes, stream) -> Tuple[torch.Tensor, torch.Tensor]:
    n, H, W = a.shape
    rank = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    total = torch.empty(1, dtype=torch.int32, device=a.device)
    _lib.check(_lib.lib().rmem_label_tube_index(tubes.data_ptr(), n, H, W, rank.data_ptr(), total.data_ptr(), stream.cuda_stream),
               'rmem_label_tube_index')
    return rank, total


def _piece_stats(a, roots, conn, stream) -> torch.Tensor:
    n, H, W = a.shape
    stats = torch.empty(n, H * W, 4, dtype=torch.int32, device=a.device)
    table = torch.empty(n, 256, 3, dtype=torch.int32, device=a.device)
    _stats(a, roots, conn, stats, table, stream)
    return stats


def _table(a, roots, stats, tubes, rank, rows, stream) -> torch.Tensor:
    n, H, W = a.shape
    table = torch.empty(max(rows, 1), 10, dtype=torch.int32, device=a.device)
    _lib.check(_lib.lib().rmem_label_tube_table(a.data_ptr(), roots.data_ptr(), stats.data_ptr(), tubes.data_ptr(), rank.data_ptr(), n, H, W,
                                                rows, table.data_ptr(), stream.cuda_stream), 'rmem_label_tube_table')
    return table


def _raise_status(what: str, bits: int):
    if bits:
        raise RmemError(f'{what}: a bounded loop of the component or tube kernels ran out (status {bits}: '
                        f'{", ".join(s for b, s in ((1, "union"), (2, "find")) if bits & b)}); this is a bug')


def label_tubes(labels_u8: torch.Tensor, connectivity: int = 8, temporal: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(tubes int32 [n, H, W], status int32 [1]) on the device: tubes[f, y, x] is the global index f' * H * W + y' * W + x' of the
    first voxel, in frame-major raster order, of the tube of (f, y, x) -- the voxels that hold the same value and are joined by the
    pieces of label_components under `connectivity` and by their links over consecutive frames under `temporal` (1: a shared pixel,
    9: two pixels at most one apart in y and x): the 3-D connected components of every value under the matching 3 x 3 x 3 structure.
    An object that leaves and comes back is one value and two tubes.  Every value counts, 0 included.  status stays 0; a set bit
    says that a bounded loop ran out (a bug).  labels_u8: uint8 device stack [n, H, W] or [H, W], taken whole.  No host sync."""
    what = 'tubes.label_tubes'
    a, conn, temp, stream = _args(what, labels_u8, connectivity, temporal)
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    tubes = _tubes(a, _roots(a, conn, status, stream), temp, status, stream)
    a.record_stream(stream)
    return tubes, status


def lineage(labels_u8: torch.Tensor, connectivity: int = 8, temporal: int = 1) -> torch.Tensor:
    """links int32 [n, H * W, 4] on the device: at the flat index of a piece's root (label_components) the smallest and largest
    root among the pieces linked to it on the frame before and on the frame after, (prev_min, prev_max, next_min, next_max), with
    (H * W, -1) for none; (H * W, -1, H * W, -1) anywhere else.  Equal min and max: exactly one neighbour in time; different:
    several -- the piece merges from, or splits into, more than one.  The stack is taken whole.  No host sync."""
    what = 'tubes.lineage'
    a, conn, temp, stream = _args(what, labels_u8, connectivity, temporal)
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    links = _links(a, _roots(a, conn, status, stream), temp, stream)
    a.record_stream(stream)
    return links


def piece_events(labels_u8: torch.Tensor, connectivity: int = 8, temporal: int = 1) -> torch.Tensor:
    """events int32 [n, 256, 4] on the device: per frame f and value v the number of pieces of v on f that are born (f >= 1, no
    predecessor), ended (f <= n - 2, no successor), splitting (several successors) and merging (several predecessors).  A cut
    object shows as splitting on the frame before the cut; a blob that appears beside it shows as born.  The stack is taken whole.
    No host sync."""
    what = 'tubes.piece_events'
    a, conn, temp, stream = _args(what, labels_u8, connectivity, temporal)
    n, H, W = a.shape
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    roots = _roots(a, conn, status, stream)
    links = _links(a, roots, temp, stream)
    events = torch.empty(n, 256, 4, dtype=torch.int32, device=a.device)
    _lib.check(_lib.lib().rmem_label_tube_events(a.data_ptr(), roots.data_ptr(), links.data_ptr(), n, H, W, events.data_ptr(),
                                                 stream.cuda_stream), 'rmem_label_tube_events')
    a.record_stream(stream)
    return events


def tube_table(labels_u8: torch.Tensor, connectivity: int = 8, temporal: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(table int32 [T, 10] on the device, tubes): one row per tube in ascending id, (first, value, voxels, pieces, f_first,
    f_last, nb_min, nb_max, border, peak_area) -- the tube's id (its first voxel), its value, its voxel and piece counts, its first
    and last frame, the extrema of its pieces' neighbouring values ((256, -1): no piece has a neighbour), 1 if a piece touches its
    frame's edge, and the area of its largest piece.  tubes is label_tubes' tensor.  The stack is taken whole.  One 4-byte
    readback, for T."""
    what = 'tubes.tube_table'
    a, conn, temp, stream = _args(what, labels_u8, connectivity, temporal)
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    roots = _roots(a, conn, status, stream)
    tubes = _tubes(a, roots, temp, status, stream)
    rank, total = _index(a, tubes, stream)
    stats = _piece_stats(a, roots, conn, stream)
    T = int(total.item())
    table = _table(a, roots, stats, tubes, rank, T, stream)[:T]
    a.record_stream(stream)
    return table, tubes


def clean_tubes(labels_u8: torch.Tensor, min_frames: int = 0, max_hole_frames: int = 0, connectivity: int = 8, temporal: int = 1,
                out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The stack (uint8, the shape of labels_u8) without its flicker, one pass in which every decision is taken from the INPUT's
    pieces and tubes.  With life = f_last - f_first + 1 of a voxel's tube, and closed = the tube begins after frame 0 and ends
    before the last frame (frame 0 is the given annotation and never changes; a tube alive on the last frame has a life nobody has
    seen the end of), a voxel of value v becomes
      flicker       v != 0, closed, life < min_frames -> the one value around its piece on that frame, else 0 (clean_labels'
                    replacement): a blob that lives for a frame or two goes, whatever its area; a small object that stays, stays;
      hole in time  v == 0, closed, life <= max_hole_frames, the tube touches no frame's edge and has one value around it -> that
                    value: a gap inside one object that is open for a few frames only is filled with the object;
      and v otherwise.  min_frames <= 1 with max_hole_frames = 0 is the identity.
    labels_u8: uint8 device stack [n, H, W] or [H, W], taken whole (tubes cross any boundary a pass would draw).  out: None
    allocates, labels_u8 itself cleans in place, any other uint8 device tensor of the same shape is written.  status: None -- one
    8-byte readback (the status word and the number of tubes, which sizes the table), RmemError if a kernel's bounded loop ran
    out; a caller's int32 [1] device tensor is OR-ed into instead (the caller zeroes it) and the call makes no host sync -- the
    table then has a row per voxel, 40 more bytes per voxel."""
    what = 'tubes.clean_tubes'
    conn, temp = _connectivity(what, connectivity), _temporal(what, temporal)
    life, hole = _count(what, 'min_frames', min_frames), _count(what, 'max_hole_frames', max_hole_frames)
    if out is not None and (not isinstance(out, torch.Tensor) or not isinstance(labels_u8, torch.Tensor) or out.shape != labels_u8.shape):
        raise RmemError(f'{what}: out must be a tensor of the labels\' shape (got {tuple(getattr(out, "shape", ()))} for '
                        f'{tuple(getattr(labels_u8, "shape", ()))})')
    a = _whole(what, labels_u8)
    n, H, W = a.shape
    if out is None:
        dst = torch.empty_like(a)
    else:
        if out.dtype != torch.uint8 or out.device != a.device or not out.is_contiguous():
            raise RmemError(f'{what}: out must be a contiguous uint8 tensor on the labels\' device')
        if out.data_ptr() == labels_u8.data_ptr() and not labels_u8.is_contiguous():
            raise RmemError(f'{what}: cleaning in place needs a contiguous stack')
        dst = out.view(a.shape)
    stream = torch.cuda.current_stream(a.device)
    own_status = status is None
    word = torch.zeros(2, dtype=torch.int32, device=a.device) if own_status else None       # (status, total): one readback
    st = word[:1] if own_status else _status(what, status, a.device)
    roots = _roots(a, conn, st, stream)
    tubes = _tubes(a, roots, temp, st, stream)
    stats = _piece_stats(a, roots, conn, stream)
    if own_status:
        rank = torch.empty(a.shape, dtype=torch.int32, device=a.device)
        _lib.check(_lib.lib().rmem_label_tube_index(tubes.data_ptr(), n, H, W, rank.data_ptr(), word[1:].data_ptr(), stream.cuda_stream),
                   'rmem_label_tube_index')
        bits, rows = (int(v) for v in word.tolist())
        _raise_status(what, bits)
    else:
        rank, _ = _index(a, tubes, stream)
        rows = n * H * W
    table = _table(a, roots, stats, tubes, rank, rows, stream)
    _lib.check(_lib.lib().rmem_label_tube_clean(a.data_ptr(), dst.data_ptr(), roots.data_ptr(), stats.data_ptr(), tubes.data_ptr(),
                                                rank.data_ptr(), table.data_ptr(), n, H, W, life, hole, stream.cuda_stream),
               'rmem_label_tube_clean')
    for t in (a, dst, st):
        t.record_stream(stream)
    return dst.view(labels_u8.shape) if out is None else out
