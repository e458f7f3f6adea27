"""Exact Euclidean distance transform of label stacks on the device, and what is built on it: the peaks of a distance map per
key value, and the Hausdorff distance of every object of two stacks (include/rmem.h: rmem_label_edt, rmem_label_edt_peaks); and
the nearest-site feature transform, which says WHICH pixel the nearest site is and reads the label there (rmem_label_nearest:
nearest, grow), with its image-aware twin, whose metric is the cheapest path through the frame's pixel grid
(rmem_label_geodesic_*: geodesic_nearest, geodesic_grow).

All distances are SQUARED distances between pixel centres as int32 (the geodesic twin's are integer path costs): exact, no float
anywhere on the device.  2^31 - 1 (SENTINEL) stands where there is nothing to measure a distance to.  Everything runs on the current stream; the stacks never leave the device.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import MAX_SIDE  # noqa: F401  (part of this module's interface)
from ._labels import frames_per_pass, geometry, int_in, is_int, like_labels, stack as _frames, stack_pair
from ._lib import RmemError

SENTINEL = 2 ** 31 - 1
MAX_D2 = 2 ** 30                             # csrc/label_nearest.hip: kMaxD2, above every real squared distance


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
    n, H, W = geometry(what, a)
    if out is None:
        dist2 = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    else:
        dist2 = like_labels(what, out, 'out', torch.int32, labels_u8, a)
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
    n, H, W = geometry(what, a)
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


# ------------------------------------------------------------------------------------------------- nearest site, grow
def _value_set(what: str, name: str, values) -> frozenset:
    """an iterable of integers in 0..255 as a set; anything else raises"""
    if isinstance(values, (str, bytes, torch.Tensor)) or not isinstance(values, Iterable):
        raise RmemError(f'{what}: {name} must be an iterable of integers in 0..255 (got {values!r})')
    vals = list(values)
    for v in vals:
        if not is_int(v) or not 0 <= int(v) <= 255:
            raise RmemError(f'{what}: {name} must be an iterable of integers in 0..255 (got {v!r} in it)')
    return frozenset(int(v) for v in vals)


def _bits(values) -> C.Array:
    """the set as rmem_label_nearest takes it: eight 32-bit words, bit (v & 31) of word v >> 5"""
    w = (C.c_uint * 8)()
    for v in values:
        w[v >> 5] |= 1 << (v & 31)
    return w


def _limit(what: str, max_distance, max_d2) -> int:
    """max_d2 as the entry point takes it: -1 without a limit; max_distance = r is max_d2 = int(r * r)"""
    if max_distance is not None and max_d2 is not None:
        raise RmemError(f'{what}: give max_distance or max_d2, not both')
    if max_d2 is not None:
        return int_in(what, 'max_d2', max_d2, 0, MAX_D2, 'None or an integer in')
    if max_distance is None:
        return -1
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating)) \
            or not math.isfinite(max_distance) or max_distance < 0:
        raise RmemError(f'{what}: max_distance must be None or a finite number that is not negative (got {max_distance!r})')
    r = float(max_distance)
    return int(min(r * r, float(MAX_D2)))                            # no real squared distance reaches 2^30


def _nearest(a, sites, fill, max_d2, index, dist2, taken, stream):
    n, H, W = a.shape
    L = _lib.lib()
    ws = workspace('nearest', a.device, stream, int(L.rmem_label_nearest_workspace_bytes(n, H, W)))
    _lib.check(L.rmem_label_nearest(a.data_ptr(), n, H, W, _bits(sites), None if fill is None else _bits(fill), max_d2,
                                    None if index is None else index.data_ptr(), None if dist2 is None else dist2.data_ptr(),
                                    None if taken is None else taken.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream),
               'rmem_label_nearest')
    for t in (a, index, dist2, taken):
        if t is not None:
            t.record_stream(stream)


def nearest(labels_u8: torch.Tensor, sites, max_distance: Optional[float] = None, max_d2: Optional[int] = None,
            return_distance: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(index, dist2), both int32 on the device and shaped like labels_u8 ([n, H, W] or [H, W]); dist2 is None with
    return_distance=False.  A pixel is a SITE if its value is in `sites` (an iterable of integers in 0..255; empty: no sites).
      index  the flat index y * W + x, within its frame, of the site nearest to the pixel by squared Euclidean distance between
             pixel centres, AMONG EQUALLY NEAR SITES THE ONE WITH THE SMALLEST FLAT INDEX (the first in raster order); -1 where the
             frame holds no site within the limit.  A site maps to itself.  scipy's distance_transform_edt(return_indices=True)
             returns one of the equally near sites, not always this one.
      dist2  that squared distance, SENTINEL where index is -1: label_edt(value=v)'s map for sites = {v} without a limit.
    The limit: max_d2 (an integer in 0..2^30; a site at exactly max_d2 still counts), or max_distance = r for max_d2 = int(r * r);
    giving both is refused, neither means no limit.  With a limit no scan is longer than its root.  H and W at most 16384.  The
    vertical offsets live in a workspace per (device, stream).  Two launches on the current stream, no host sync."""
    what = 'distance.nearest'
    s = _value_set(what, 'sites', sites)
    d2max = _limit(what, max_distance, max_d2)
    a = _frames(what, labels_u8)
    geometry(what, a)
    index = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    dist2 = torch.empty(a.shape, dtype=torch.int32, device=a.device) if return_distance else None
    _nearest(a, s, None, d2max, index, dist2, None, torch.cuda.current_stream(a.device))
    return index.view(labels_u8.shape), None if dist2 is None else dist2.view(labels_u8.shape)


def grow(labels_u8: torch.Tensor, fill=(0,), sites=None, max_distance: Optional[float] = None, max_d2: Optional[int] = None,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 stack like labels_u8 on the device: every pixel whose value is in `fill` takes the value of its nearest site (nearest's
    rule, ties to the smallest flat index) if there is one within the limit; every other pixel keeps its value.  sites: the values
    that are sites; None: every value not in `fill`.  A value in both sets stays where it is (a site maps to itself); a value in
    neither (a void label, say) is neither overwritten nor spread.  fill = (0,) grows the objects over the background without
    ever overwriting one another; fill = (255,) with sites=None replaces a void label by the nearest real value.  max_distance /
    max_d2: as nearest.  out: None allocates; a contiguous uint8 device tensor of the labels' shape that is not the labels is
    written.  Only the stack is asked of the kernel: pixels outside `fill` are copied without a scan.  Two launches on the
    current stream, no host sync."""
    what = 'distance.grow'
    f = _value_set(what, 'fill', fill)
    s = frozenset(range(256)) - f if sites is None else _value_set(what, 'sites', sites)
    d2max = _limit(what, max_distance, max_d2)
    a = _frames(what, labels_u8)
    geometry(what, a)
    if out is None:
        taken = torch.empty(a.shape, dtype=torch.uint8, device=a.device)
    else:
        taken = like_labels(what, out, 'out', torch.uint8, labels_u8, a)
        if out.data_ptr() == a.data_ptr():
            raise RmemError(f'{what}: out must not be the labels (they are read at the nearest site while out is written)')
    _nearest(a, s, f, d2max, None, None, taken, torch.cuda.current_stream(a.device))
    return taken.view(labels_u8.shape) if out is None else out


# ------------------------------------------------------------------------------------------------- geodesic nearest site, grow
MAX_COST = 2 ** 30                           # csrc/label_geodesic.hip: kMaxCost, above every real path cost


def geodesic_tile() -> Tuple[int, int]:
    """(th, tw): the core tile of a round of the geodesic transform"""
    th, tw = C.c_int(), C.c_int()
    _lib.check(_lib.lib().rmem_label_geodesic_tile(C.byref(th), C.byref(tw)), 'rmem_label_geodesic_tile')
    return th.value, tw.value


def _image(what: str, image_u8, labels_u8: torch.Tensor, a: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(the frames as [n, H, W, C], C) of the image that goes with labels_u8 (whose stack view is a): [n, H, W] grey or
    [n, H, W, C] with stacked labels, [H, W] or [H, W, C] with 2-D ones; C is 1 or 3"""
    if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8:
        raise RmemError(f'{what}: image must be a uint8 tensor')
    if image_u8.device != a.device:
        raise RmemError(f'{what}: image must be on the labels\' device (got {image_u8.device} and {a.device})')
    ls = tuple(labels_u8.shape)
    if tuple(image_u8.shape) == ls:
        channels = 1
    elif image_u8.dim() == len(ls) + 1 and tuple(image_u8.shape[:-1]) == ls and image_u8.shape[-1] in (1, 3):
        channels = int(image_u8.shape[-1])
    else:
        raise RmemError(f'{what}: image must have the labels\' shape {ls}, grey, or that with 1 or 3 interleaved channels after it '
                        f'(got {tuple(image_u8.shape)})')
    if not image_u8.is_contiguous():
        raise RmemError(f'{what}: image must be contiguous')
    return image_u8.view(a.shape + (channels,)), channels


def _cost_limit(what: str, max_cost) -> int:
    return -1 if max_cost is None else int_in(what, 'max_cost', max_cost, 0, MAX_COST, 'None or an integer in')


def _geodesic(what, a, img, channels, sites, fill, spatial, colour, limit, index, cost, taken, batch, workspace_bytes, info):
    """begin, calls of `batch` rounds until no tile of a call's last round changed, finish; in passes of as many frames as fit"""
    n, H, W = a.shape
    L = _lib.lib()
    per_frame = int(L.rmem_label_geodesic_workspace_bytes(1, H, W))
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]
    stream = torch.cuda.current_stream(a.device)
    ws = workspace('geodesic', a.device, stream, int(L.rmem_label_geodesic_workspace_bytes(k, H, W)))
    changed = torch.empty(k, dtype=torch.int32, device=a.device)
    sbits, fbits = _bits(sites), None if fill is None else _bits(fill)
    if isinstance(info, dict):
        info.update(rounds=0, calls=0, passes=[])
    for f0 in range(0, n, k):
        la, im = a[f0:f0 + k], img[f0:f0 + k]
        m = la.shape[0]
        need = int(L.rmem_label_geodesic_workspace_bytes(m, H, W))
        _lib.check(L.rmem_label_geodesic_begin(la.data_ptr(), m, H, W, sbits, ws.data_ptr(), need, stream.cuda_stream), 'rmem_label_geodesic_begin')
        rounds = calls = 0
        while True:
            _lib.check(L.rmem_label_geodesic_rounds(im.data_ptr(), channels, m, H, W, spatial, colour, limit, rounds, batch, changed.data_ptr(),
                                                    ws.data_ptr(), need, stream.cuda_stream), 'rmem_label_geodesic_rounds')
            rounds, calls = rounds + batch, calls + 1
            if not changed[:m].cpu().any():                                # the one readback of the call
                break
            if rounds > H * W + batch:                                     # every round that changes something makes a pixel final
                raise RmemError(f'{what}: the rounds did not come to rest after {rounds} rounds on frames of {H} x {W}')
        out = [None if t is None else t[f0:f0 + k].data_ptr() for t in (index, cost, taken)]
        _lib.check(L.rmem_label_geodesic_finish(la.data_ptr(), m, H, W, fbits, limit, rounds, out[0], out[1], out[2], ws.data_ptr(), need,
                                                stream.cuda_stream), 'rmem_label_geodesic_finish')
        if isinstance(info, dict):
            info['rounds'] += rounds
            info['calls'] += calls
            info['passes'].append({'frames': m, 'rounds': rounds, 'calls': calls})
    for t in (a, img, index, cost, taken):
        if t is not None:
            t.record_stream(stream)


def _geodesic_args(what, labels_u8, image_u8, spatial, colour, max_cost, batch):
    sp, co = int_in(what, 'spatial', spatial, 1, 64), int_in(what, 'colour', colour, 0, 64)
    limit = _cost_limit(what, max_cost)
    b = int_in(what, 'batch', batch, 1, 2 ** 20)
    a = _frames(what, labels_u8)
    geometry(what, a)
    img, channels = _image(what, image_u8, labels_u8, a)
    return a, img, channels, sp, co, limit, b


def geodesic_nearest(labels_u8: torch.Tensor, image_u8: torch.Tensor, sites, spatial: int = 1, colour: int = 1, max_cost: Optional[int] = None,
                     return_cost: bool = True, batch: int = 8, workspace_bytes: Optional[int] = None,
                     info: Optional[dict] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(index, cost), both int32 on the device and shaped like labels_u8 ([n, H, W] or [H, W]); cost is None with
    return_cost=False.  nearest's image-aware twin: the SITES are the pixels whose value is in `sites`, but the nearest one is the
    site with the cheapest path through the 8-connected pixel grid, where the step between neighbours p and q costs
        spatial * s + colour * sum over the channels of |I(p) - I(q)|,   s = 5 for an axial step, 7 for a diagonal one
    (integers: spatial in 1..64, colour in 0..64; colour = 0 is the 5-7 chamfer distance).
      index  the flat index y * W + x, within its frame, of the site with the smallest (cost, index); -1 where no site is within
             max_cost.  A site maps to itself.
      cost   that cost, SENTINEL where index is -1.
    image_u8: uint8, contiguous, on the labels' device: the labels' shape (grey) or that with 1 or 3 interleaved channels after it
    ([n, H, W, 3]: what jpeg.overlay takes).  max_cost: None or an integer in 0..2^30; a cost == max_cost still counts, and tiles
    no front reaches do no work.  The transform runs in rounds over tiles (geodesic_tile): calls of `batch` rounds until no tile
    changed in a call's last round, one readback of 4 bytes per frame per call; a call that reports a change lowered a key and
    keys are bounded below, so the loop ends.  The result does not depend on batch.  The two key planes (16 bytes per pixel)
    live in a workspace per (device, stream) of as many frames as fit workspace_bytes (default: 256 MiB, or one frame's need
    where that is larger); a longer stack goes through in passes.  info, a dict, receives {'rounds': rounds launched, 'calls':
    calls of rounds, 'passes': [per pass]}.  H and W at most 16384.  The current stream."""
    what = 'distance.geodesic_nearest'
    s = _value_set(what, 'sites', sites)
    a, img, channels, sp, co, limit, b = _geodesic_args(what, labels_u8, image_u8, spatial, colour, max_cost, batch)
    index = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    cost = torch.empty(a.shape, dtype=torch.int32, device=a.device) if return_cost else None
    _geodesic(what, a, img, channels, s, None, sp, co, limit, index, cost, None, b, workspace_bytes, info)
    return index.view(labels_u8.shape), None if cost is None else cost.view(labels_u8.shape)


def geodesic_grow(labels_u8: torch.Tensor, image_u8: torch.Tensor, fill=(0,), sites=None, spatial: int = 1, colour: int = 1,
                  max_cost: Optional[int] = None, out: Optional[torch.Tensor] = None, batch: int = 8, workspace_bytes: Optional[int] = None,
                  info: Optional[dict] = None) -> torch.Tensor:
    """uint8 stack like labels_u8 on the device: grow under geodesic_nearest's metric.  Every pixel whose value is in `fill` takes
    the value of the site with the smallest (cost, index) if one is within max_cost; every other pixel keeps its value.  sites:
    None: every value not in `fill`.  A region grown from a seed stops where the frame changes, not halfway to the next seed.
    out: None allocates; a contiguous uint8 device tensor of the labels' shape that is not the labels is written.  image_u8,
    spatial, colour, max_cost, batch, workspace_bytes, info: as geodesic_nearest."""
    what = 'distance.geodesic_grow'
    f = _value_set(what, 'fill', fill)
    s = frozenset(range(256)) - f if sites is None else _value_set(what, 'sites', sites)
    a, img, channels, sp, co, limit, b = _geodesic_args(what, labels_u8, image_u8, spatial, colour, max_cost, batch)
    if out is None:
        taken = torch.empty(a.shape, dtype=torch.uint8, device=a.device)
    else:
        taken = like_labels(what, out, 'out', torch.uint8, labels_u8, a)
        if out.data_ptr() == a.data_ptr():
            raise RmemError(f'{what}: out must not be the labels (they are read at the winning site while out is written)')
    _geodesic(what, a, img, channels, s, f, sp, co, limit, None, None, taken, b, workspace_bytes, info)
    return taken.view(labels_u8.shape) if out is None else out
