"""Label stacks traced into polygons on the device: the outer contours and the holes of every object of every frame.

Labelling tools take polygons -- CVAT and Labelme tracks, COCO `segmentation` lists -- and propagating a first-frame annotation
through a clip is what a semi-supervised VOS engine is used for outside the benchmarks.  trace turns a uint8 label stack into
closed rings of pixel corners without leaving the device (include/rmem.h, rmem_label_polygons, has the contract: edges, the
successor rule, rings, vertices, area2); trace_label_stack is the host-side product, with every hole attached to its outer ring
through the connected components (components.label_components); evaluator.polygon_results is the COCO-shaped twin of rle_results.
Replaces labels.cpu() and a sequential border follower per frame and object: only the rings and vertices cross to the host.

    rings, verts, counts = polygons.trace(labels, num_objs)                     # device tensors, no host sync
    per_frame = polygons.trace_label_stack(labels, num_objs, squeeze_idx=idx)   # [{object id: [{'exterior', 'area2', 'holes'}]}]
    per_frame = evaluator.polygon_results(labels, num_objs, idx, holes='drop')  # [{object id: {'size', 'segmentation', 'area'}}]
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import connectivity as _connectivity, frames_per_pass, int_in, is_int, object_keys, stack as _frames
from ._lib import RmemError

ST_CAPACITY, ST_LINK, ST_ORDER = 1, 2, 4     # include/rmem.h
MAX_EDGES = 2 ** 31 - 1


def unit() -> int:
    """pixels of one row the walk kernel gives a thread: where its units' seams lie"""
    return int(_lib.lib().rmem_label_polygons_unit())


def default_max_edges(n: int, H: int, W: int) -> int:
    """The edge capacity `trace` takes when the caller names none: per frame a quarter of its pixels plus four times H + W.  An
    estimate, not a bound -- a checkerboard has 4 H W edges per frame, noise about 3 per object pixel: the outline of a blob grows
    with the root of its area, so blob-like masks with speckle fit many times over, and when the edges do not fit, the status word
    says so and counts[0] still gives the exact number."""
    return int(max(4, min(n * (H * W // 4 + 4 * (H + W) + 64), 4 * n * H * W, MAX_EDGES)))


def _max_edges(what: str, max_edges, n: int, H: int, W: int) -> int:
    if max_edges is None:
        return default_max_edges(n, H, W)
    if not is_int(max_edges) or not 4 <= int(max_edges) <= MAX_EDGES:
        raise RmemError(f'{what}: max_edges must be an integer in 4..2^31-1 (got {max_edges!r})')
    return int(max_edges)


def trace(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8,
          max_edges: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rings int32 [max_edges // 4 + 1, 8], verts int32 [max_edges, 2], counts int32 [4]) on the device, of a uint8 device stack
    [n, H, W] or [H, W] whose objects are the values 1..num_objs under `connectivity` (4 or 8).  counts = (edges E, rings R,
    vertices V, status); rings[:R] = (frame, value, first vertex, vertex count, area2, start edge id, edge count, 0) in the order
    (frame, start edge), area2 positive for an outer ring and negative for a hole; verts[:V] = (x, y) pixel corners, ring after
    ring.  Rows beyond R and V are not written.  max_edges: default_max_edges when None; status is ST_CAPACITY when the stack has
    more edges: counts is (E, 0, 0, ST_CAPACITY) then, E exact.  Any other status bit is a bug.  One call of rmem_label_polygons
    on the current stream, no host sync; the workspace is one buffer per (device, stream) that only grows."""
    what = 'polygons.trace'
    K, conn = int_in(what, 'num_objs', num_objs, 1, 255), _connectivity(what, connectivity)
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    M = _max_edges(what, max_edges, n, H, W)
    L = _lib.lib()
    nbytes = int(L.rmem_label_polygons_workspace_bytes(n, H, W, M))
    if nbytes == 0:
        raise RmemError(f'{what}: bad geometry (at most 65535 frames, H * W at most 2^26, max_edges at least 4; got {n}x{H}x{W}, {M})')
    dev = a.device
    stream = torch.cuda.current_stream(dev)
    ws = workspace('polygons', dev, stream, nbytes)
    rings = torch.empty(M // 4 + 1, 8, dtype=torch.int32, device=dev)
    verts = torch.empty(M, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    _lib.check(L.rmem_label_polygons(a.data_ptr(), n, H, W, K, conn, M, ws.data_ptr(), ws.numel(), rings.data_ptr(), verts.data_ptr(),
                                     counts.data_ptr(), stream.cuda_stream), 'rmem_label_polygons')
    a.record_stream(stream)
    return rings, verts, counts


def group_rings(rings: np.ndarray, verts: np.ndarray, n: int, num_objs: int, squeeze_idx: Optional[Sequence[int]] = None,
                roots_at_start: Optional[np.ndarray] = None) -> List[Dict]:
    """trace_label_stack's grouping, pure host code: rings [R, 8] and verts [V, 2] of n frames as
    `trace` orders them -> one dict per frame, {key of object id: [{'exterior', 'area2', 'holes'}, ...]} with an empty list for an
    object the frame does not hold.  roots_at_start [R]: label_components' root at every ring's start pixel; a hole (area2 < 0)
    goes to the outer ring of its frame whose start pixel is that root.  None: holes are not attached, see trace_label_stack."""
    key = object_keys(int(num_objs), squeeze_idx)
    frames: List[Dict] = [{k: [] for k in key.values()} for _ in range(n)]
    if roots_at_start is None:
        for fr in frames:
            fr[None] = {'holes': {k: [] for k in key.values()}}
    outer = {}
    rows = [(int(r[0]), int(r[1]), verts[int(r[2]):int(r[2]) + int(r[3])].astype(np.int32, copy=True), int(r[4]), int(r[5]) >> 2)
            for r in rings]
    for f, v, ring, area2, pixel in rows:
        if area2 > 0:
            poly = {'exterior': ring, 'area2': area2, 'holes': []}
            outer[(f, pixel)] = poly
            if v in key:
                frames[f][key[v]].append(poly)
    for k, (f, v, ring, area2, pixel) in enumerate(rows):
        if area2 > 0:
            continue
        if roots_at_start is None:
            if v in key:
                frames[f][None]['holes'][key[v]].append(ring)
            continue
        poly = outer.get((f, int(roots_at_start[k])))
        if poly is None:
            raise RmemError(f'polygons: the hole of value {v} that starts at pixel {pixel} of frame {f} has no outer ring at '
                            f'its component\'s first pixel {int(roots_at_start[k])}; this is a bug')
        poly['area2'] += area2
        poly['holes'].append(ring)
    return frames


def frame_bytes(H: int, W: int, parents: bool = True) -> int:
    """what trace_label_stack counts per frame of a pass: the workspace and the outputs of `trace` at default_max_edges, and the
    roots of the components where holes get parents"""
    M = default_max_edges(1, H, W)
    ws = int(_lib.lib().rmem_label_polygons_workspace_bytes(1, H, W, M))
    if ws == 0:
        raise RmemError(f'polygons: bad geometry (H * W at most 2^26; got {H}x{W})')
    return ws + 16 * M + 32 + (4 * H * W if parents else 0)


def _status_text(bits: int) -> str:
    return ', '.join(s for b, s in ((ST_LINK, 'a successor was not found'), (ST_ORDER, 'a ring position out of range')) if bits & b)


def trace_label_stack(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8, squeeze_idx: Optional[Sequence[int]] = None,
                      parents: bool = True, max_edges: Optional[int] = None, workspace_bytes: Optional[int] = None) -> List[Dict]:
    """Per frame of a uint8 device label stack [n, H, W] or [H, W]: {object id: [polygon, ...]} for the objects 1..num_objs, one
    polygon per connected piece (`connectivity`) in the order of the pieces' first pixels, an empty list for an object the frame
    does not hold.  polygon = {'exterior': int32 [k, 2], 'area2': int, 'holes': [int32 [k, 2], ...]}: rings of (x, y) pixel
    corners, y down, the object on the right of the direction of travel (include/rmem.h); 'area2' is twice the piece's pixel count
    (the exterior's shoelace sum plus its holes' negative ones).  squeeze_idx: the keys are squeeze_idx[id] (save_masks'
    un-squeeze); ids beyond its length are left out.
    parents=True attaches every hole to its outer ring through the connected components: components.label_components with the
    same connectivity, and one device gather of the root at every ring's start pixel (start edge >> 2) -- an outer ring starts at
    side 0 of its piece's first raster pixel, which is that root.  parents=False skips the components: every polygon's 'holes' is
    empty and its 'area2' is the exterior's alone, and the frame's dict has one more key, None, with {'holes': {object id: [int32
    [k, 2], ...]}}, the holes of every object in start-edge order.
    The stack goes in passes of as many frames as keep the workspace and outputs of one `trace` call at or below workspace_bytes
    (default: 256 MiB, or one frame's need where that is larger).  Per pass: one readback of counts, then one readback of the used
    rows.  max_edges (per pass; default: default_max_edges): when the status says ST_CAPACITY the pass is traced once more with
    max_edges = counts[0]."""
    what = 'polygons.trace_label_stack'
    K, conn = int_in(what, 'num_objs', num_objs, 1, 255), _connectivity(what, connectivity)
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    per_frame = frame_bytes(H, W, parents)
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]     # at least 1: the budget holds a frame
    if max_edges is not None:
        _max_edges(what, max_edges, n, H, W)
    out: List[Dict] = []
    for f0 in range(0, n, k):
        part = a[f0:f0 + k]
        m = part.shape[0]
        rings, verts, counts = trace(part, K, conn, max_edges)
        roots = cc_status = None
        if parents:
            from .components import label_components
            roots, cc_status = label_components(part, conn)
        c = counts.cpu().tolist()
        if c[3] & ST_CAPACITY:
            if c[0] >= MAX_EDGES:
                raise RmemError(f'{what}: {m} frames of {H} x {W} have 2^31 - 1 edges or more; give fewer frames a pass (workspace_bytes)')
            rings, verts, counts = trace(part, K, conn, max(4, c[0]))
            c = counts.cpu().tolist()
        if c[3]:
            raise RmemError(f'{what}: the tracer failed (status {c[3]}: {_status_text(c[3])}); this is a bug')
        R, V = c[1], c[2]
        used = [rings[:R].reshape(-1), verts[:V].reshape(-1)]
        if parents:
            at = rings[:R, 0].long() * (H * W) + (rings[:R, 5] >> 2).long()
            used += [roots.view(-1)[at], cc_status]
        host = torch.cat(used).cpu().numpy()                         # the one readback of the used rows
        at_start = None
        if parents:
            if int(host[-1]):
                raise RmemError(f'{what}: a bounded loop of the component kernels ran out (status {int(host[-1])}); this is a bug')
            at_start = host[8 * R + 2 * V:8 * R + 2 * V + R]
        out += group_rings(host[:8 * R].reshape(R, 8), host[8 * R:8 * R + 2 * V].reshape(V, 2), m, K, squeeze_idx, at_start)
    return out


def coco_polygons(frames: List[Dict], size: Tuple[int, int], holes: str = 'rings') -> List[Dict]:
    """evaluator.polygon_results' shaping of trace_label_stack's output (parents=True), pure host code"""
    H, W = int(size[0]), int(size[1])
    out = []
    for fr in frames:
        entry = {}
        for k, polys in fr.items():
            e = {'size': [H, W], 'segmentation': [p['exterior'].reshape(-1).tolist() for p in polys]}
            if holes == 'rings':
                e['holes'] = [h.reshape(-1).tolist() for p in polys for h in p['holes']]
                e['area'] = sum(p['area2'] for p in polys) // 2
            else:
                e['area'] = sum(p['area2'] - sum(_area2(h) for h in p['holes']) for p in polys) // 2
            entry[k] = e
        out.append(entry)
    return out


def _area2(ring: np.ndarray) -> int:
    x, y = ring[:, 0].astype(np.int64), ring[:, 1].astype(np.int64)
    return int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
