"""What shape an object has, from uint8 label stacks on the device (include/rmem.h, rmem_label_moments and the hull entry points;
csrc/label_shapes.hip): raw moments, row extents, convex hulls, and on the host the region properties derived from them.

  label_moments   int64 [n, 256, 6] = (count, sum x, sum y, sum x^2, sum x y, sum y^2) per frame and label value; exact.
  row_extents     int32 [n, num_objs, H, 2] = (xmin, xmax) of every object on every image row.
  convex_hulls    the hull of every object's pixel SQUARES, in pixel-corner coordinates (polygons.trace's system, so hull area >=
                  pixel count), from the row extents alone; canonical rings, so two of them can be compared for equality.
  props_from_tables / region_props
                  centroid, central moments, orientation, axis lengths, eccentricity, solidity, extent, Feret diameter and the
                  minimum-area rectangle (VOT's rotated box) per frame and object.

Replaces labels.cpu() and numpy / scipy / OpenCV per frame and object: only the moment table and the hull vertices cross to the
host.  Everything up to the float properties is integer-exact.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import frames_per_pass, geometry, int_in, is_int, object_keys, stack as _frames
from ._lib import RmemError


def _stream(a: torch.Tensor) -> torch.cuda.Stream:
    return torch.cuda.current_stream(a.device)


def _rows(a: torch.Tensor, num: int, moments, extents, stream) -> None:
    n, H, W = a.shape
    _lib.check(_lib.lib().rmem_label_moments(a.data_ptr(), n, H, W, num, None if moments is None else moments.data_ptr(),
                                             None if extents is None else extents.data_ptr(), stream.cuda_stream), 'rmem_label_moments')
    a.record_stream(stream)


def label_moments(labels_u8: torch.Tensor) -> torch.Tensor:
    """int64 [n, 256, 6] on the device: (m00, m10, m01, m20, m11, m02) = (count, sum x, sum y, sum x^2, sum x y, sum y^2) of the
    pixels of every frame of a uint8 device stack [n, H, W] or [H, W] that equal every label value, x and y the pixel's column
    and row index; zeros for a value the frame does not hold.  H and W at most 16384.  Exact and bit-reproducible.  One call on
    the current stream, no host sync."""
    what = 'shapes.label_moments'
    a = _frames(what, labels_u8)
    n, H, W = geometry(what, a)
    out = torch.empty(n, 256, 6, dtype=torch.int64, device=a.device)
    _rows(a, 0, out, None, _stream(a))
    return out


def row_extents(labels_u8: torch.Tensor, num_objs: int) -> torch.Tensor:
    """int32 [n, num_objs, H, 2] on the device: (xmin, xmax) of the object v = 1..num_objs (entry v - 1) on every image row of
    every frame, (W, -1) on a row that lacks it.  One call on the current stream, no host sync."""
    what = 'shapes.row_extents'
    K = int_in(what, 'num_objs', num_objs, 1, 255)
    a = _frames(what, labels_u8)
    n, H, W = geometry(what, a)
    out = torch.empty(n, K, H, 2, dtype=torch.int32, device=a.device)
    _rows(a, K, None, out, _stream(a))
    return out


def frame_bytes(H: int, num_objs: int) -> int:
    """what convex_hulls keeps per frame of a pass: the row extents and the two flag bits of every corner level"""
    return 8 * num_objs * H + ((num_objs * (H + 1) + 15) & ~15)


def _workspace_arg(what: str, workspace_bytes) -> None:
    """what can be said of workspace_bytes before the stack is looked at; frames_per_pass compares it with one frame's need"""
    if workspace_bytes is not None and (not is_int(workspace_bytes) or workspace_bytes < 1):
        raise RmemError(f'{what}: workspace_bytes must be a positive integer or None (got {workspace_bytes!r})')


def _hulls(a: torch.Tensor, K: int, workspace_bytes, moments: Optional[torch.Tensor], what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    n, H, W = geometry(what, a)
    per_frame = frame_bytes(H, K)
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s extents and flags')[1]
    L, dev, stream = _lib.lib(), a.device, _stream(a)
    ws = workspace('shapes', dev, stream, k * per_frame)
    ext, flags = ws[:8 * K * H * k].view(torch.int32), ws[8 * K * H * k:]
    offsets = torch.empty(n * K + 1, dtype=torch.int32, device=dev)
    s = stream.cuda_stream

    def count(f0: int, m: int, mom, counts: torch.Tensor) -> None:
        _rows(a[f0:f0 + m], K, None if mom is None else mom[f0:f0 + m], ext, stream)
        _lib.check(L.rmem_label_hull_count(ext.data_ptr(), m, H, W, K, flags.data_ptr(), counts.data_ptr(), s), 'rmem_label_hull_count')

    for f0 in range(0, n, k):
        count(f0, min(k, n - f0), moments, offsets[f0 * K:])
    _lib.check(L.rmem_label_hull_offsets(offsets.data_ptr(), n * K, s), 'rmem_label_hull_offsets')
    V = int(offsets[n * K].item())                                  # the one readback: the total
    if not 0 <= V <= 2 * (H + 1) * n * K:
        raise RmemError(f'{what}: {V} hull vertices for {n * K} objects of at most {H} rows; this is a bug')
    verts = torch.empty(V, 2, dtype=torch.int32, device=dev)
    if V:
        again = torch.empty(k * K, dtype=torch.int32, device=dev) if k < n else None
        for f0 in range(0, n, k):
            m = min(k, n - f0)
            if k < n:                                               # several passes: the workspace holds another pass's tables
                count(f0, m, None, again)                           # the counts once more, beside the scanned ones
            _lib.check(L.rmem_label_hull_write(ext.data_ptr(), flags.data_ptr(), m, H, W, K, offsets[f0 * K:].data_ptr(), verts.data_ptr(),
                                               V, s), 'rmem_label_hull_write')
    return verts, offsets


def convex_hulls(labels_u8: torch.Tensor, num_objs: int, workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(verts int32 [V, 2], offsets int32 [n * num_objs + 1]) on the device: the convex hull of the pixel squares of every object
    1..num_objs of every frame of a uint8 device stack [n, H, W] or [H, W]; the ring of object v of frame f is
    verts[offsets[o]:offsets[o + 1]] with o = f * num_objs + v - 1, empty for an absent object.  A ring holds (x, y) pixel corners
    (polygons.trace's coordinates), strictly convex vertices only, starts at the vertex with the smallest (y, x) and travels east
    along the top edge first -- the object on the right, y down, trace's outer rings: polygons._area2 is positive.  An object h
    rows high has at most 2 (h + 1) vertices.
    From the row extents alone (include/rmem.h has the method).  The stack goes in passes of as many frames as keep the extents
    and flags at or below workspace_bytes (default: 256 MiB, or one frame's need where that is larger); with several passes the
    extents are computed twice.  The current stream; one 4-byte readback (the total V)."""
    what = 'shapes.convex_hulls'
    K = int_in(what, 'num_objs', num_objs, 1, 255)
    _workspace_arg(what, workspace_bytes)
    return _hulls(_frames(what, labels_u8), K, workspace_bytes, None, what)


def _min_rect(ring: np.ndarray) -> Tuple[np.ndarray, float]:
    """the minimum-area rectangle around a convex ring of integer points [k, 2]: one side lies on an edge; per edge e the ranges
    of p . e and e x p over the ring are exact integers (int64: each below 2^30, their product below 2^60) and the area is their
    product over |e|^2; the minimum by cross-multiplying Python ints (int64 would overflow), the first edge on a tie"""
    p = ring.astype(np.int64)
    e = np.roll(p, -1, axis=0) - p
    dots = p @ e.T                                                  # [point, edge]
    crosses = p[:, 1:2] * e[None, :, 0] - p[:, 0:1] * e[None, :, 1]
    d0, d1, c0, c1 = dots.min(axis=0), dots.max(axis=0), crosses.min(axis=0), crosses.max(axis=0)
    nums, dens = ((d1 - d0) * (c1 - c0)).tolist(), (e * e).sum(axis=1).tolist()
    best = 0
    for i in range(1, len(nums)):
        if nums[i] * dens[best] < nums[best] * dens[i]:
            best = i
    ex, ey, den = int(e[best, 0]), int(e[best, 1]), dens[best]
    lo_d, hi_d, lo_c, hi_c = int(d0[best]), int(d1[best]), int(c0[best]), int(c1[best])
    # the point with p . e = d and e x p = c is (d e + c (-ey, ex)) / |e|^2
    corners = np.array([[(d * ex - c * ey) / den, (d * ey + c * ex) / den] for d, c in ((lo_d, lo_c), (hi_d, lo_c), (hi_d, hi_c), (lo_d, hi_c))],
                       dtype=np.float64)
    return corners, nums[best] / den


def _feret2(ring: np.ndarray) -> int:
    p = ring.astype(np.int64)
    d = p[:, None, :] - p[None, :, :]
    return int((d * d).sum(axis=2).max())


def props_from_tables(moments: np.ndarray, verts: np.ndarray, offsets: np.ndarray, n: int, num_objs: int, H: int, W: int,
                      squeeze_idx: Optional[Sequence[int]] = None) -> List[Dict]:
    """[{key: props} per frame] from HOST copies of label_moments' and convex_hulls' tables, pure numpy and Python ints; keys are
    the object ids 1..num_objs or squeeze_idx[id] (_labels.object_keys); an object the frame does not hold is left out.  props:
      area            m00, int
      centroid        (x, y) = (m10 / m00, m01 / m00)
      mu              (m00 m20 - m10^2, m00 m11 - m10 m01, m00 m02 - m01^2): the exact integer numerators of the central moments
                      mu20, mu11, mu02 (each is the entry over m00^2); Python ints
      orientation     0.5 atan2(2 mu11, mu20 - mu02), from +x towards +y (y down), 0 when both arguments are 0
      major_axis, minor_axis   4 sqrt(lambda) of the eigenvalues of [[mu20, mu11], [mu11, mu02]]
      eccentricity    sqrt(1 - lambda_min / lambda_max), 0 for a single pixel
      hull            int32 [k, 2], convex_hulls' ring; hull_area2: its shoelace sum (twice the area), int
      solidity        2 area / hull_area2
      extent          area over the area of the axis-aligned box (from the hull's range)
      feret2          the largest squared distance between two hull vertices, int
      min_rect        float64 [4, 2], the corners of the minimum-area rectangle around the hull in ring direction, the first side
                      on the hull edge that gives it (the first such edge on a tie); min_rect_area
    Pixels are POINT MASSES at their integer indices, as in scikit-image's regionprops: the 1/12 a uniform unit square would add
    to mu20 and mu02 is not added, so a single pixel has axis lengths 0."""
    what = 'shapes.props_from_tables'
    K = int_in(what, 'num_objs', num_objs, 1, 255)
    moments, verts, offsets = np.asarray(moments), np.asarray(verts), np.asarray(offsets)
    if moments.shape != (n, 256, 6) or offsets.shape != (n * K + 1,) or verts.ndim != 2 or verts.shape[1] != 2:
        raise RmemError(f'{what}: moments [n, 256, 6], verts [V, 2] and offsets [n * num_objs + 1] are required '
                        f'(got {moments.shape}, {verts.shape}, {offsets.shape})')
    keys = object_keys(K, squeeze_idx)
    out: List[Dict] = []
    for f in range(n):
        fr = {}
        for v, key in keys.items():
            m00, m10, m01, m20, m11, m02 = (int(t) for t in moments[f, v])
            if m00 == 0:
                continue
            o = f * K + v - 1
            ring = verts[int(offsets[o]):int(offsets[o + 1])].astype(np.int32, copy=True)
            if len(ring) < 4:
                raise RmemError(f'{what}: object {v} of frame {f} has {m00} pixels and a hull of {len(ring)} vertices')
            p = [(int(x), int(y)) for x, y in ring]
            mu = (m00 * m20 - m10 * m10, m00 * m11 - m10 * m01, m00 * m02 - m01 * m01)
            u20, u11, u02 = (t / (m00 * m00) for t in mu)
            root = math.sqrt((u20 - u02) ** 2 + 4.0 * u11 * u11)
            l1, l2 = (u20 + u02 + root) / 2.0, max((u20 + u02 - root) / 2.0, 0.0)
            hull_area2 = sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(p, p[1:] + p[:1]))
            xs, ys = [x for x, _ in p], [y for _, y in p]
            corners, rect_area = _min_rect(ring)
            fr[key] = dict(area=m00, centroid=(m10 / m00, m01 / m00), mu=mu, orientation=0.5 * math.atan2(2 * mu[1], mu[0] - mu[2]),
                           major_axis=4.0 * math.sqrt(l1), minor_axis=4.0 * math.sqrt(l2),
                           eccentricity=0.0 if l1 == 0 else math.sqrt(max(1.0 - l2 / l1, 0.0)),
                           hull=ring, hull_area2=hull_area2, solidity=2 * m00 / hull_area2,
                           extent=m00 / ((max(xs) - min(xs)) * (max(ys) - min(ys))),
                           feret2=_feret2(ring),
                           min_rect=corners, min_rect_area=rect_area)
        out.append(fr)
    return out


def region_props(labels_u8: torch.Tensor, num_objs: int, squeeze_idx: Optional[Sequence[int]] = None,
                 workspace_bytes: Optional[int] = None) -> List[Dict]:
    """props_from_tables of a uint8 device stack [n, H, W] or [H, W]: the moments come from the same pass over the labels as the
    row extents, the hulls from those, and the moment table, the offsets and the vertices cross to the host in one readback (after
    convex_hulls' 4 bytes)."""
    what = 'shapes.region_props'
    K = int_in(what, 'num_objs', num_objs, 1, 255)
    _workspace_arg(what, workspace_bytes)
    a = _frames(what, labels_u8)
    n, H, W = geometry(what, a)
    moments = torch.empty(n, 256, 6, dtype=torch.int64, device=a.device)
    verts, offsets = _hulls(a, K, workspace_bytes, moments, what)
    host = torch.cat([moments.view(torch.int32).reshape(-1), offsets, verts.reshape(-1)]).cpu().numpy()
    nm = n * 256 * 12
    return props_from_tables(host[:nm].view(np.int64).reshape(n, 256, 6), host[nm + n * K + 1:].reshape(-1, 2), host[nm:nm + n * K + 1],
                             n, K, H, W, squeeze_idx)
