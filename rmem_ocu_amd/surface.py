"""Surface distances of two label stacks on the device: the robust numbers reported next to J and F -- the 95th-percentile
Hausdorff distance, the average symmetric surface distance and the surface Dice at a tolerance (include/rmem.h: rmem_label_surface,
rmem_label_edt_at, rmem_surface_census).

The SURFACE of value v in a frame is the set of pixels that hold v and have a 4-neighbour that holds another value or lies outside
the frame.  For object i = 1..num_objs, stacks a and b, the SAMPLES of a frame are the squared distances (int32, between pixel
centres) of every surface pixel of a to the nearest surface pixel of b (set 0), the mirror image (set 1), and both pooled (set 2);
2^31 - 1 (SENTINEL) where the other surface is empty.  The CENSUS reduces every set to nine integers on the device
(FIELDS); one readback of that table yields every metric.  Everything on the device is integer: bit-reproducible.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import MAX_SIDE, frames_per_pass, geometry, int_in, like_labels, stack as _frames, stack_pair
from ._lib import RmemError
from .distance import SENTINEL

FIELDS = ('count', 'sum_fix', 'max', 'lo', 'hi', 'within0', 'within1', 'within2', 'within3')
MAX_TOL2 = 2 ** 30 - 1


def _surface(a, out, stream):
    n, H, W = a.shape
    _lib.check(_lib.lib().rmem_label_surface(a.data_ptr(), n, H, W, out.data_ptr(), stream.cuda_stream), 'rmem_label_surface')


def _edt_at(labels, keys, value, key, samples, g, stream):
    n, H, W = labels.shape
    _lib.check(_lib.lib().rmem_label_edt_at(labels.data_ptr(), keys.data_ptr(), n, H, W, value, key, samples.data_ptr(), g.data_ptr(), g.numel(),
                                            stream.cuda_stream), 'rmem_label_edt_at')


def _tol2(what: str, tol2) -> list:
    if not isinstance(tol2, (tuple, list)) or len(tol2) > 4:
        raise RmemError(f'{what}: tol2 must be a tuple of at most 4 integers (got {tol2!r})')
    return [int_in(what, 'every tol2', t, 0, MAX_TOL2) for t in tol2]


def label_surface(labels_u8: torch.Tensor) -> torch.Tensor:
    """uint8 device stack of the labels' shape: labels on the surface pixels (a 4-neighbour holds another value or lies outside
    the frame), 0 elsewhere -- for every value v, (labels == v) & ~binary_erosion(labels == v, cross, border_value=0).  Background
    pixels are therefore always 0; a void label of 255 is an ordinary value.  labels_u8: [n, H, W] or [H, W], H and W at most 16384.
    One launch on the current stream, no host sync."""
    what = 'surface.label_surface'
    a = _frames(what, labels_u8)
    geometry(what, a)
    out = torch.empty_like(a)
    stream = torch.cuda.current_stream(a.device)
    _surface(a, out, stream)
    for t in (a, out):
        t.record_stream(stream)
    return out.view(labels_u8.shape)


def edt_at(labels_u8: torch.Tensor, keys_u8: torch.Tensor, value: int, key: int, samples: torch.Tensor) -> torch.Tensor:
    """distance.label_edt(labels_u8, value) evaluated only where keys_u8 == key: there samples (int32, contiguous, the stacks' shape,
    their device) receives the squared distance to the nearest pixel of labels_u8 that holds `value`, SENTINEL where the frame holds
    none; every other entry of samples keeps what it held.  The column pass is the whole frame's; the row pass looks at the rows
    that hold a key pixel, and there at the key pixels alone.  Two launches on the current stream, no host sync.  Returns samples."""
    what = 'surface.edt_at'
    v, k = int_in(what, 'value', value, 0, 255), int_in(what, 'key', key, 0, 255)
    a, b = stack_pair(what, labels_u8, keys_u8, ('labels', 'keys'))
    for t in (a, b):
        _frames(what, t)
    n, H, W = geometry(what, a)
    like_labels(what, samples, 'samples', torch.int32, labels_u8, a)
    stream = torch.cuda.current_stream(a.device)
    g = workspace('edt', a.device, stream, int(_lib.lib().rmem_label_edt_workspace_bytes(n, H, W)))
    _edt_at(a, b, v, k, samples, g, stream)
    for t in (a, b, samples):
        t.record_stream(stream)
    return samples


def surface_census(a_u8: torch.Tensor, b_u8: torch.Tensor, num_objs: int, tol2: Sequence[int] = (), q: int = 9500,
                   workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """int64 [n, num_objs, 3, 9] on the device: for every frame, object i = 1..num_objs and set (0: surface of a to surface of b,
    1: b to a, 2: both pooled) the FIELDS of the set's samples:
      count    m, the number of samples, sentinels included;       sum_fix  the sum of floor(sqrt(d2 * 2^32)): distances with 16
      max      the largest d2;                                               fractional bits, each rounded down;
      lo, hi   the samples of rank r_lo = (m - 1) * q // 10000 and r_hi = min(r_lo + 1, m - 1) in ascending order (q: hundredths of
               a percent, 0..10000): with frac = ((m - 1) * q % 10000) / 10000, sqrt(lo) + frac * (sqrt(hi) - sqrt(lo)) is numpy's
               linear percentile of the distances;
      within   the number of samples with d2 <= tol2[t], for up to 4 tolerances in 0..2^30 - 1; 0 for unused t.
    An empty set is (0, 0, -1, -1, -1, 0, 0, 0, 0); a set of sentinels (the other surface is empty) (m, 0, SENTINEL, SENTINEL,
    SENTINEL, 0, 0, 0, 0).  a_u8, b_u8: uint8 device stacks of one shape, [n, H, W] or [H, W].  Two surface launches, per object two
    sampled transforms (sites in one surface stack, keys in the other) into two sample stacks all objects share -- surfaces of
    different objects are disjoint pixels -- and one census.  Surfaces, samples, vertical distances and the census' tables live in a
    workspace per (device, stream) of as many frames as fit workspace_bytes (default: 256 MiB, or one frame's need where that is
    larger); the call walks the stacks that many frames at a time.  No host sync."""
    what = 'surface.surface_census'
    K = int_in(what, 'num_objs', num_objs, 1, 255)
    tols = _tol2(what, tol2)
    qq = int_in(what, 'q', q, 0, 10000)
    a, b = stack_pair(what, a_u8, b_u8)
    for t in (a, b):
        _frames(what, t)
    n, H, W = geometry(what, a)
    L = _lib.lib()
    HW = H * W
    c1, g1 = int(L.rmem_surface_census_workspace_bytes(1, K)), int(L.rmem_label_edt_workspace_bytes(1, H, W))
    per_frame = c1 + 2 * HW * 4 + g1 + 2 * HW                          # the census' tables, two sample stacks, g, two surface stacks
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]
    stream = torch.cuda.current_stream(a.device)
    ws = workspace('surface_census', a.device, stream, k * per_frame)
    o = [0, k * c1, k * c1 + k * HW * 4, k * c1 + 2 * k * HW * 4, k * c1 + 2 * k * HW * 4 + k * g1]      # widest alignment first
    cws, g = ws[o[0]:o[1]], ws[o[3]:o[4]]
    da, db = (ws[o[i]:o[i + 1]].view(torch.int32).view(k, H, W) for i in (1, 2))
    sa, sb = (ws[o[4] + i * k * HW:o[4] + (i + 1) * k * HW].view(k, H, W) for i in (0, 1))
    table = torch.empty(n, K, 3, 9, dtype=torch.int64, device=a.device)
    tol_arr = (C.c_int * 4)(*tols)
    for f0 in range(0, n, k):
        m = min(k, n - f0)
        _surface(a[f0:f0 + m], sa, stream)
        _surface(b[f0:f0 + m], sb, stream)
        for i in range(1, K + 1):
            _edt_at(sb[:m], sa[:m], i, i, da, g, stream)             # to the surface of b, read on the surface of a
            _edt_at(sa[:m], sb[:m], i, i, db, g, stream)
        _lib.check(L.rmem_surface_census(da.data_ptr(), sa.data_ptr(), db.data_ptr(), sb.data_ptr(), m, H, W, K, tol_arr, len(tols), qq,
                                         table[f0:f0 + m].data_ptr(), cws.data_ptr(), cws.numel(), stream.cuda_stream), 'rmem_surface_census')
    for t in (a, b):
        t.record_stream(stream)
    return table


def metrics_from_table(table: np.ndarray, q: int, num_tol: int, pooled: bool = True) -> Dict[str, np.ndarray]:
    """surface_metrics' dict from a census table on the host (int64 [n, num_objs, 3, 9], taken with the same q and num_tol
    tolerances)"""
    t = np.asarray(table, dtype=np.int64)
    count, mx = t[..., 0], t[..., 2]
    empty, lone = count == 0, mx == SENTINEL                         # per set: no sample; the other surface is empty
    safe = np.maximum(count, 1).astype(np.float64)

    def root(v):
        return np.sqrt(np.where(empty | lone, 0, v).astype(np.float64))

    def finish(v, s):                                                # 0 where there is nothing to measure, inf where one side is missing
        return np.where(lone[..., s], np.inf, np.where(empty[..., s], 0.0, v))

    frac = ((count - 1) * q % 10000).astype(np.float64) / 10000.0
    lo, hi = root(t[..., 3]), root(t[..., 4])
    pct = lo + frac * (hi - lo)
    one_sided = lone[..., 0] | lone[..., 1]
    if pooled:
        hd95 = finish(pct[..., 2], 2)
    else:
        hd95 = np.where(one_sided, np.inf, np.maximum(np.where(empty[..., 0], 0.0, pct[..., 0]), np.where(empty[..., 1], 0.0, pct[..., 1])))
    within = t[..., 2, 5:5 + num_tol].astype(np.float64) / safe[..., 2, None]
    return {'hd': finish(root(mx)[..., 2], 2),
            'hd95': hd95,
            'assd': finish(t[..., 2, 1].astype(np.float64) / safe[..., 2] / 65536.0, 2),
            'nsd': np.where(empty[..., 2, None], 1.0, within)}


def surface_metrics(a_u8: torch.Tensor, b_u8: torch.Tensor, num_objs: int, tolerances: Sequence[float] = (1.0, 2.0),
                    percentile: float = 95.0, pooled: bool = True) -> Dict[str, np.ndarray]:
    """dict of float64 numpy arrays [n, num_objs], distances in pixels between the surfaces of object i = 1..num_objs of two stacks:
      hd    the Hausdorff distance of the two surfaces (the root of the pooled max);
      hd95  the `percentile`-th percentile (numpy's linear rule; hundredths of a percent at the finest) of the pooled distances;
            pooled=False: the larger of the two directed percentiles;
      assd  the average symmetric surface distance: the mean of the pooled distances (each rounded down to 2^-16 pixels);
      nsd   [n, num_objs, len(tolerances)]: the surface Dice, the share of the pooled samples within the tolerance tau (up to 4,
            in pixels; d2 <= floor(tau^2)).
    Where both surfaces are empty the distances are 0 and nsd is 1; where exactly one is, the distances are inf and nsd is 0.
    surface_census on the device, one readback of its table."""
    what = 'surface.surface_metrics'
    if not isinstance(tolerances, (tuple, list)) or len(tolerances) > 4:
        raise RmemError(f'{what}: tolerances must be a tuple of at most 4 numbers (got {tolerances!r})')
    tols = []
    for tau in tolerances:
        if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)) or not (tau >= 0 and tau * tau <= MAX_TOL2):
            raise RmemError(f'{what}: every tolerance must be a number in 0..{MAX_SIDE * 2 - 1} pixels (got {tau!r})')
        tols.append(int(math.floor(tau * tau)))
    pc = percentile
    if isinstance(pc, bool) or not isinstance(pc, (int, float, np.integer, np.floating)) or not 0 <= pc <= 100 \
            or abs(pc * 100 - round(pc * 100)) > 1e-6:
        raise RmemError(f'{what}: percentile must be a number in 0..100 in hundredths of a percent (got {percentile!r})')
    q = int(round(pc * 100))
    table = surface_census(a_u8, b_u8, num_objs, tuple(tols), q).cpu().numpy()
    return metrics_from_table(table, q, len(tols), bool(pooled))
