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

Traced rings are pixel staircases; simplify thins them on the device under a tolerance in pixels (include/rmem.h,
rmem_polygon_simplify, has the contract: Douglas-Peucker against the segment, exact in 64-bit integers, 1/16 pixel steps).  Every
dropped vertex is within the tolerance of the simplified ring, and filling the simplified rings back changes no pixel whose centre
is farther than the tolerance from every ring edge of its frame.  Topology is NOT preserved: a simplified ring may touch or cross
itself or a neighbour, as with OpenCV's approxPolyDP; the even-odd fill takes such rings as they come.

    rings_s, verts_s, counts_s = polygons.simplify(rings, verts, counts, 1.0)   # device tensors, no host sync
    per_frame = polygons.trace_label_stack(labels, num_objs, tolerance=1.0)     # the same dicts with tens of vertices per ring

The other direction: annotation polygons filled into a uint8 label stack on the device (include/rmem.h,
rmem_polygon_fill_labels, has the contract: the even-odd rule sampled at pixel centres, exact on 1/256-pixel fixed point, left
and top edges inclusive; what `trace` emits fills back to exactly the pixels it came from).  PackedPolygons quantises and flattens
a clip's shapes on the host; only their edges cross to the device.  Replaces a host rasteriser per frame and object and the upload
of H * W bytes per frame.  Not pycocotools' frPoly (a five times upsampled outline with its own rounding), nor Pillow's
ImageDraw.polygon (which also draws the outline): masks can differ from either in boundary pixels.

    gt = polygons.fill_label_stack(frames, (H, W), device)                      # frames[f] = {label value: shape}; uint8 [n, H, W]
    gt, ids = evaluator.labels_from_polygons(frames, (H, W), device)            # frames[f] = {track id: shape}; value i + 1 = ids[i]
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import Packed, stream_of, workspace
from ._labels import MAX_FRAMES, MAX_PIXELS, WORKSPACE_CAP, connectivity as _connectivity, frames_per_pass, int_in, is_int, object_keys, stack as _frames
from ._lib import RmemError

ST_CAPACITY, ST_LINK, ST_ORDER = 1, 2, 4     # include/rmem.h
MAX_EDGES = 2 ** 31 - 1
TOLERANCE_STEPS, MAX_TOLERANCE = 16, 64      # simplify: steps per pixel and the largest tolerance, in pixels
SIMPLIFY_ST_TABLE, SIMPLIFY_ST_RING = 8, 16
FILL_ST_DESC, FILL_ST_PREFIX, FILL_ST_EDGE = 1, 2, 4
FILL_STATUS_NAMES = {FILL_ST_DESC: 'bad shape table entry, or an edge of a shape outside the pass',
                     FILL_ST_PREFIX: 'the crossing prefix disagrees with an edge',
                     FILL_ST_EDGE: 'an edge coordinate out of range or a crossing outside the shape\'s box'}
FIXED = 256                                  # fixed-point steps per pixel
MAX_COORD = 2 ** 20                          # |x|, |y| of a vertex, in pixels
MAX_CROSSINGS = 2 ** 31 - 1
SHAPE_DTYPE = np.dtype([('frame', '<i4'), ('value', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('plane', '<i8')])   # RmemPolyShape


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


def short_max() -> int:
    """vertices of the longest ring that `simplify` gives one wave: where its two kernels' seam lies"""
    return int(_lib.lib().rmem_polygon_simplify_short_max())


def _steps(what: str, tolerance) -> int:
    """T of include/rmem.h: rint(16 * tolerance) of a finite number in 0..64"""
    if not _is_number(tolerance) or not 0 <= float(tolerance) <= MAX_TOLERANCE:         # NaN fails both comparisons
        raise RmemError(f'{what}: tolerance must be a finite number in 0..{MAX_TOLERANCE} pixels (got {tolerance!r})')
    return int(np.rint(TOLERANCE_STEPS * float(tolerance)))


def simplify(rings: torch.Tensor, verts: torch.Tensor, counts: torch.Tensor, tolerance: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rings_s, verts_s, counts_s) on the device, shaped like the inputs: the table of `trace` -- or any int32 table of that form
    -- with every ring thinned by Douglas-Peucker under `tolerance` pixels (0..64, rounded to 1/16; include/rmem.h,
    rmem_polygon_simplify, has the rule).  rings_s[:R] are the input's rows with the new first vertex, the kept count and, in
    column 7, the original count; area2 stays the TRACED area.  verts_s[:V_out] are the kept vertices, ring after ring; counts_s =
    (V, R, V_out, status).  Rows beyond R and V_out are not written.  A non-zero status of the input is passed on with R = V_out =
    0; SIMPLIFY_ST_TABLE: counts that do not fit the tensors; SIMPLIFY_ST_RING: a bad ring row or a coordinate outside 0..32767,
    that ring has 0 vertices.  Every dropped vertex is within the tolerance of the segment between its kept neighbours; topology
    is NOT preserved: a simplified ring may touch or cross itself or a neighbour.  One call on the current stream, no host sync;
    the workspace is one buffer per (device, stream) that only grows."""
    what = 'polygons.simplify'
    T = _steps(what, tolerance)
    for name, t, cols in (('rings', rings, 8), ('verts', verts, 2), ('counts', counts, None)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise RmemError(f'{what}: {name} must be an int32 tensor')
        if not t.is_contiguous() or (t.dim() != 2 or t.shape[1] != cols or t.shape[0] < 1 if cols else tuple(t.shape) != (4,)):
            raise RmemError(f'{what}: {name} must be a contiguous ' + (f'[k, {cols}] tensor, k >= 1' if cols else '[4] tensor')
                            + f' (got {tuple(t.shape)}, strides {tuple(t.stride())})')
    if not rings.device == verts.device == counts.device:
        raise RmemError(f'{what}: rings, verts and counts must be on one device')
    if not rings.is_cuda:
        raise RmemError(f'{what}: rings, verts and counts must be device tensors (there is no host simplifier)')
    MR, MV = rings.shape[0], verts.shape[0]
    L = _lib.lib()
    nbytes = int(L.rmem_polygon_simplify_workspace_bytes(MR, MV))
    if nbytes == 0:
        raise RmemError(f'{what}: at most 2^31 - 1 rings and vertices (got {MR}, {MV})')
    dev = rings.device
    stream = torch.cuda.current_stream(dev)
    ws = workspace('polygons.simplify', dev, stream, nbytes)
    rings_s, verts_s, counts_s = torch.empty_like(rings), torch.empty_like(verts), torch.empty_like(counts)
    _lib.check(L.rmem_polygon_simplify(rings.data_ptr(), verts.data_ptr(), counts.data_ptr(), MR, MV, T, ws.data_ptr(), ws.numel(),
                                       rings_s.data_ptr(), verts_s.data_ptr(), counts_s.data_ptr(), stream.cuda_stream),
               'rmem_polygon_simplify')
    for t in (rings, verts, counts):
        t.record_stream(stream)
    return rings_s, verts_s, counts_s


def drop_degenerate(frames: List[Dict]) -> List[Dict]:
    """trace_label_stack's degenerate='drop', pure host code, in place: an exterior with fewer than 3 vertices or a zero shoelace
    sum leaves with its holes; so does such a hole (under the key None too)"""
    def alive(ring):                                                # plain integers: most rings have a handful of vertices
        if len(ring) < 3:
            return False
        p = ring.tolist()
        return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(p, p[1:] + p[:1])) != 0
    for fr in frames:
        for k, polys in fr.items():
            if k is None:
                polys['holes'] = {o: [h for h in hs if alive(h)] for o, hs in polys['holes'].items()}
                continue
            polys[:] = [p for p in polys if alive(p['exterior'])]
            for p in polys:
                p['holes'] = [h for h in p['holes'] if alive(h)]
    return frames


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


def frame_bytes(H: int, W: int, parents: bool = True, simplified: bool = False) -> int:
    """what trace_label_stack counts per frame of a pass: the workspace and the outputs of `trace` at default_max_edges, the
    roots of the components where holes get parents, and the workspace and the outputs of `simplify` where a tolerance is given"""
    M = default_max_edges(1, H, W)
    ws = int(_lib.lib().rmem_label_polygons_workspace_bytes(1, H, W, M))
    if ws == 0:
        raise RmemError(f'polygons: bad geometry (H * W at most 2^26; got {H}x{W})')
    more = int(_lib.lib().rmem_polygon_simplify_workspace_bytes(M // 4 + 1, M)) + 16 * M + 32 if simplified else 0
    return ws + 16 * M + 32 + (4 * H * W if parents else 0) + more


def _status_text(bits: int) -> str:
    return ', '.join(s for b, s in ((ST_LINK, 'a successor was not found'), (ST_ORDER, 'a ring position out of range')) if bits & b)


def trace_label_stack(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8, squeeze_idx: Optional[Sequence[int]] = None,
                      parents: bool = True, max_edges: Optional[int] = None, workspace_bytes: Optional[int] = None,
                      tolerance: Optional[float] = None, degenerate: str = 'drop') -> List[Dict]:
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
    max_edges = counts[0].
    tolerance (pixels, 0..64; None: the traced rings as they are): `simplify` is launched directly behind `trace`, both count
    vectors come back in the pass's one counts readback, the capacity retry traces and simplifies again, and the used rows that
    come back are the simplified tables'.  'area2' stays the TRACED pixel area.  Topology is NOT preserved: simplified rings may
    touch or cross themselves or each other.  degenerate='drop' (only with a tolerance) then removes every exterior with fewer
    than 3 kept vertices or a zero shoelace sum together with its holes, and every such hole; 'keep' leaves everything."""
    what = 'polygons.trace_label_stack'
    K, conn = int_in(what, 'num_objs', num_objs, 1, 255), _connectivity(what, connectivity)
    if tolerance is not None:
        _steps(what, tolerance)
    if degenerate not in ('drop', 'keep'):
        raise RmemError(f'{what}: degenerate must be \'drop\' or \'keep\' (got {degenerate!r})')
    a = _frames(what, labels_u8)
    n, H, W = a.shape
    per_frame = frame_bytes(H, W, parents, tolerance is not None)
    k = frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s need')[1]     # at least 1: the budget holds a frame
    if max_edges is not None:
        _max_edges(what, max_edges, n, H, W)
    out: List[Dict] = []
    for f0 in range(0, n, k):
        part = a[f0:f0 + k]
        m = part.shape[0]
        def traced(cap):
            """trace, simplify behind it where asked, and the one readback of the counts of both"""
            t = trace(part, K, conn, cap)
            if tolerance is None:
                return t, t[2].cpu().tolist(), None
            s = simplify(*t, tolerance)
            both = torch.cat([t[2], s[2]]).cpu().tolist()
            return s, both[:4], both[4:]

        (rings, verts, counts), c, cs = traced(max_edges)
        roots = cc_status = None
        if parents:
            from .components import label_components
            roots, cc_status = label_components(part, conn)
        if c[3] & ST_CAPACITY:
            if c[0] >= MAX_EDGES:
                raise RmemError(f'{what}: {m} frames of {H} x {W} have 2^31 - 1 edges or more; give fewer frames a pass (workspace_bytes)')
            (rings, verts, counts), c, cs = traced(max(4, c[0]))
        if c[3]:
            raise RmemError(f'{what}: the tracer failed (status {c[3]}: {_status_text(c[3])}); this is a bug')
        R, V = c[1], c[2]
        if cs is not None:
            if cs[3] or cs[1] != R:
                raise RmemError(f'{what}: the simplifier failed (status {cs[3]}, {cs[1]} of {R} rings); this is a bug')
            V = cs[2]
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
    if tolerance is not None and degenerate == 'drop':
        drop_degenerate(out)
    return out


def coco_polygons(frames: List[Dict], size: Tuple[int, int], holes: str = 'rings', simplified: bool = False) -> List[Dict]:
    """evaluator.polygon_results' shaping of trace_label_stack's output (parents=True), pure host code.  simplified: 'area' is
    the shoelace area of the rings the entry lists, a float (exteriors minus the listed holes under 'rings', exteriors alone under
    'drop'); otherwise the pixel count from the traced 'area2'."""
    H, W = int(size[0]), int(size[1])
    out = []
    for fr in frames:
        entry = {}
        for k, polys in fr.items():
            e = {'size': [H, W], 'segmentation': [p['exterior'].reshape(-1).tolist() for p in polys]}
            if holes == 'rings':
                e['holes'] = [h.reshape(-1).tolist() for p in polys for h in p['holes']]
            if simplified:
                inner = sum(_area2(h) for p in polys for h in p['holes']) if holes == 'rings' else 0     # negative: holes run the other way
                e['area'] = (sum(_area2(p['exterior']) for p in polys) + inner) / 2.0
            elif holes == 'rings':
                e['area'] = sum(p['area2'] for p in polys) // 2
            else:
                e['area'] = sum(p['area2'] - sum(_area2(h) for h in p['holes']) for p in polys) // 2
            entry[k] = e
        out.append(entry)
    return out


def _area2(ring: np.ndarray) -> int:
    x, y = ring[:, 0].astype(np.int64), ring[:, 1].astype(np.int64)
    return int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


# ---------------------------------------------------------------------------------------------------------------- filling

def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _is_pair(v) -> bool:
    return isinstance(v, (list, tuple, np.ndarray)) and len(v) == 2 and all(_is_number(c) for c in v)


def _ring(r, where: str) -> np.ndarray:
    """float64 [k, 2], k >= 3, of a ring given as [k, 2] or flat"""
    try:
        a = np.asarray(r, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is not None and a.ndim == 1:
        if a.size % 2:
            raise RmemError(f'PackedPolygons: {where}: a flat ring of {a.size} numbers (x0, y0, x1, y1, ...: an even count)')
        a = a.reshape(-1, 2)
    if a is None or a.ndim != 2 or a.shape[1] != 2:
        raise RmemError(f'PackedPolygons: {where}: a ring is an array-like [k, 2] of (x, y) or a flat sequence x0, y0, x1, y1, ...')
    if a.shape[0] < 3:
        raise RmemError(f'PackedPolygons: {where}: a ring of {a.shape[0]} vertices (at least 3)')
    return a


def _rings_of(shape, size: Tuple[int, int], where: str) -> List[np.ndarray]:
    """the rings of a shape in any of the forms PackedPolygons takes"""
    if isinstance(shape, dict):
        if 'segmentation' in shape:
            if 'size' in shape and tuple(int(v) for v in shape['size']) != size:
                raise RmemError(f'PackedPolygons: {where}: size {list(shape["size"])} differs from the stack\'s {list(size)}')
            return [_ring(r, where) for r in list(shape['segmentation']) + list(shape.get('holes', ()))]
        if 'exterior' in shape:
            return [_ring(shape['exterior'], where)] + [_ring(h, where) for h in shape.get('holes', ())]
        raise RmemError(f'PackedPolygons: {where}: a polygon dict has \'exterior\' (and \'holes\') or \'segmentation\'')
    if isinstance(shape, np.ndarray):
        return [_ring(shape, where)] if shape.ndim <= 2 else [_ring(r, where) for r in shape]
    if isinstance(shape, (list, tuple)):
        if len(shape) == 0:
            return []
        if all(_is_number(v) for v in shape) or all(_is_pair(v) for v in shape):
            return [_ring(shape, where)]
        out: List[np.ndarray] = []
        for item in shape:
            out += _rings_of(item, size, where) if isinstance(item, dict) else [_ring(item, where)]
        return out
    raise RmemError(f'PackedPolygons: {where}: a shape is a ring, a list of rings, a polygon dict or a list of polygon dicts')


class PackedPolygons(Packed):
    """A clip's polygon annotations, packed once: frames[f] is {value: shape} or [(value, shape), ...] (listing order = painting
    order, the later shape wins where two overlap; at most 255 per frame), value the label (1..255) the shape paints.  A shape
    is a set of rings filled under the even-odd rule (include/rmem.h, rmem_polygon_fill_labels), given as one ring, a list of
    rings (an empty list paints nothing), a polygon dict of trace_label_stack ({'exterior': ring, 'holes': [ring, ...]}, other
    keys ignored), a list of such dicts (trace_label_stack(...)[f][k]), or a COCO-shaped entry {'segmentation': [flat ring, ...]}
    with an optional 'holes': [flat ring, ...] (evaluator.polygon_results(...)[f][k]; its 'size', if present, must equal size).
    A ring is an array-like [k, 2] of (x, y) -- x right, y down, pixel corners at integers, any fractions -- or a flat sequence
    x0, y0, x1, y1, ...; a list whose elements are all pairs of numbers is one [k, 2] ring.  size = (H, W) of the stack.
    Packing needs no GPU: it quantises the vertices to 1/256 pixel (numpy.rint, ties to even), flattens every shape into its edges
    that cross a sample row of the frame, and computes every shape's box and bit-plane offset and the prefix of the edges'
    crossing counts.  One pinned int32 buffer holds edge_xy [E, 4], edge_shape [E], edge_first [E + 1] and frame_shape [n + 1];
    the shape table (RmemPolyShape) is the descriptor table.  len() is the number of shapes; status words are per shape.
    Not pycocotools' frPoly rule: masks can differ from it in boundary pixels."""
    NOUN, STATUS_NAMES = 'polygon shape', FILL_STATUS_NAMES

    def __init__(self, frames: Sequence, size: Tuple[int, int]):
        self.height, self.width = H, W = int(size[0]), int(size[1])
        n = len(frames)
        if n < 1 or n > MAX_FRAMES or H < 1 or W < 1 or H * W > MAX_PIXELS:
            raise RmemError(f'PackedPolygons: {n} frames of {H}x{W} (at least one frame, at most 65535, H * W at most 2^26)')
        self.shape = torch.Size((n, H, W))
        self.where: List[Tuple[int, int]] = []
        rings: List[np.ndarray] = []
        ring_shape: List[int] = []
        for f, entry in enumerate(frames):
            items = list(entry.items()) if isinstance(entry, dict) else list(entry)
            if len(items) > 255:
                raise RmemError(f'PackedPolygons: frame {f} lists {len(items)} shapes (at most 255)')
            for value, shape in items:
                if not _is_number(value) or int(value) != value or not 1 <= int(value) <= 255:
                    raise RmemError(f'PackedPolygons: frame {f}: label value {value!r} outside 1..255')
                mine = _rings_of(shape, (H, W), f'frame {f}, value {value}')
                rings += mine
                ring_shape += [len(self.where)] * len(mine)
                self.where.append((f, int(value)))
        S = self.nshapes = len(self.where)
        lens = np.array([len(r) for r in rings], dtype=np.int64)
        V = np.concatenate(rings) if rings else np.zeros((0, 2), dtype=np.float64)
        bad = np.flatnonzero(~(np.abs(V) <= MAX_COORD).all(axis=1))            # also every NaN and infinity
        ends = np.cumsum(lens)
        if bad.size:
            f, v = self.where[ring_shape[int(np.searchsorted(ends, bad[0], side='right'))]]
            x, y = V[bad[0]]
            raise RmemError(f'PackedPolygons: frame {f}, value {v}: vertex ({x}, {y}) is not finite or beyond 2^20 pixels')
        Q = np.rint(V * FIXED).astype(np.int64)
        nxt = np.arange(len(Q), dtype=np.int64) + 1
        nxt[ends - 1] = ends - lens                                            # a ring's last vertex joins its first
        of_vertex = np.repeat(np.array(ring_shape, dtype=np.int64), lens)      # the shape of every vertex, and of the edge it starts
        table = np.zeros(S, dtype=SHAPE_DTYPE)
        table['frame'], table['value'] = [w[0] for w in self.where], [w[1] for w in self.where]
        per_shape = np.bincount(of_vertex, minlength=S)
        held = np.flatnonzero(per_shape)
        if held.size:                                                          # the pixels whose centres a shape can cover, in the frame
            at = (np.cumsum(per_shape) - per_shape)[held]
            for lo, hi, col, top in (('x0', 'x1', 0, W), ('y0', 'y1', 1, H)):
                table[lo][held] = np.clip((np.minimum.reduceat(Q[:, col], at) + 127) >> 8, 0, top)
                table[hi][held] = np.clip((np.maximum.reduceat(Q[:, col], at) + 127) >> 8, 0, top)
        empty = (table['x0'] >= table['x1']) | (table['y0'] >= table['y1'])
        for k in ('x0', 'y0', 'x1', 'y1'):
            table[k][empty] = 0
        words = (table['y1'] - table['y0']).astype(np.int64) * ((table['x1'] - table['x0'] + 31) >> 5)
        table['plane'] = np.cumsum(words) - words
        X0, Y0, X1, Y1 = Q[:, 0], Q[:, 1], Q[nxt, 0], Q[nxt, 1]
        rows = np.minimum(H, (np.maximum(Y0, Y1) + 127) >> 8) - np.maximum(0, (np.minimum(Y0, Y1) + 127) >> 8)
        keep = (rows > 0) & ~empty[of_vertex]                                  # the edges that cross a sample row of a shape with a plane
        self.edge_xy = np.stack([X0, Y0, X1, Y1], axis=1)[keep].astype(np.int32)
        self.edge_shape = of_vertex[keep].astype(np.int32)
        first = np.concatenate([[0], np.cumsum(rows[keep])])
        E = self.nedges = int(keep.sum())
        self.crossings = int(first[-1])
        if self.crossings > MAX_CROSSINGS:
            raise RmemError(f'PackedPolygons: the edges cross {self.crossings} sample rows (at most 2^31 - 1); pack fewer frames')
        self.edge_first = first.astype(np.int32)
        self.table = table
        self.frame_shape = np.searchsorted(table['frame'], np.arange(n + 1), side='left').astype(np.int32)
        self.shape_edge = np.searchsorted(self.edge_shape, np.arange(S + 1), side='left').astype(np.int64)   # the first edge of every shape
        fs = self.frame_shape.astype(np.int64)
        total = np.concatenate([[0], np.cumsum(words)])
        self.frame_words = total[fs[1:]] - total[fs[:-1]]                      # plane words per frame
        self.plane_words = int(total[-1])
        self.offsets = (0, 16 * E, 20 * E, 24 * E + 4)                         # bytes: edge_xy, edge_shape, edge_first, frame_shape
        blob = np.concatenate([self.edge_xy.reshape(-1), self.edge_shape, self.edge_first, self.frame_shape]).astype(np.int32)
        self.buf = torch.from_numpy(blob.view(np.uint8))
        self.descs = table
        self.desc_bytes = torch.from_numpy(table.view(np.uint8).reshape(-1).copy() if S else np.zeros(SHAPE_DTYPE.itemsize, dtype=np.uint8))
        if torch.cuda.is_available():                                          # packing itself needs no GPU
            self.buf, self.desc_bytes = self.buf.pin_memory(), self.desc_bytes.pin_memory()
        self._dev = {}

    def __len__(self):
        return self.nshapes

    def passes(self, workspace_bytes: Optional[int] = None) -> List[_lib.PolyPass]:
        """The passes of whole frames fill_labels_into makes: as many consecutive frames each as keep
        rmem_polygon_fill_workspace_bytes of their planes at or below workspace_bytes (default: _labels.WORKSPACE_CAP, or the
        largest frame's need where that is larger); a budget below the largest frame's need is refused."""
        need = _lib.lib().rmem_polygon_fill_workspace_bytes
        largest = int(need(int(self.frame_words.max())))
        if workspace_bytes is None:
            workspace_bytes = max(largest, min(int(need(self.plane_words)), WORKSPACE_CAP))
        elif not is_int(workspace_bytes) or workspace_bytes < largest:
            raise RmemError(f'polygons.fill_labels_into: workspace_bytes must be an integer of at least the largest frame\'s need, '
                            f'{largest} bytes (got {workspace_bytes!r})')
        n = self.shape[0]
        fs, out, f0 = self.frame_shape, [], 0
        while f0 < n:
            f1, words = f0 + 1, int(self.frame_words[f0])
            while f1 < n and int(need(words + int(self.frame_words[f1]))) <= workspace_bytes:
                words += int(self.frame_words[f1])
                f1 += 1
            s0, s1 = int(fs[f0]), int(fs[f1])
            e0, e1 = int(self.shape_edge[s0]), int(self.shape_edge[s1])
            c0, c1 = int(self.edge_first[e0]), int(self.edge_first[e1])
            plane0 = int(self.table['plane'][s0]) if s0 < self.nshapes else self.plane_words
            out.append(_lib.PolyPass(f0, f1 - f0, s0, s1 - s0, e0, e1 - e0, c0, c1 - c0, plane0, words))
            f0 = f1
        return out

    def check(self, device, first: int = 0, count: Optional[int] = None, stream=None):
        """Packed.check, naming the frame and the label value of the first bad shape as well"""
        try:
            super().check(device, first, count, stream)
        except RmemError as e:
            st = self.status(device)[first:first + (len(self) - first if count is None else count)].cpu()
            k = first + int(torch.nonzero(st).flatten()[0])
            raise RmemError(f'{e} [shape {k}: frame {self.where[k][0]}, value {self.where[k][1]}]') from None


def fill_pass(packed: PackedPolygons, dc, p: _lib.PolyPass, ws: torch.Tensor, out: torch.Tensor, raw_stream: int):
    """one call of rmem_polygon_fill_labels: pass p of `packed`, whose buffers on the device are dc, into out on a raw stream"""
    import ctypes
    n, H, W = packed.shape
    base = dc.bits.data_ptr()
    xy, shape, first, frames = (base + o for o in packed.offsets)
    _lib.check(_lib.lib().rmem_polygon_fill_labels(xy, shape, first, packed.nedges, dc.descs.data_ptr(), packed.nshapes, frames, n, H, W,
                                                   ctypes.byref(p), ws.data_ptr(), ws.numel(), out.data_ptr(), dc.status.data_ptr(),
                                                   raw_stream), 'rmem_polygon_fill_labels')


def fill_labels_into(packed: PackedPolygons, out: torch.Tensor, stream=None, workspace_bytes: Optional[int] = None):
    """Every frame of `packed` into out (uint8 [n, H, W], contiguous, device) on ``stream`` (a torch.cuda.Stream or a raw handle;
    default: the current stream).  Nothing waits for the GPU: the pack is copied from pinned memory on the stream, the status
    words land in packed.status(device) and are read later by packed.check(device).  The frames go in passes of whole frames
    whose bit planes fit workspace_bytes (PackedPolygons.passes: 256 MiB by default, or the largest frame's need); a smaller
    budget is refused.  A pack without any shape zero-fills out."""
    what = 'polygons.fill_labels_into'
    if not isinstance(packed, PackedPolygons):
        raise RmemError(f'{what}: packed must be a PackedPolygons')
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda:
        raise RmemError(f'{what}: out must be a uint8 device tensor')
    if tuple(out.shape) != tuple(packed.shape) or not out.is_contiguous():
        raise RmemError(f'{what}: out must be a contiguous {list(packed.shape)} tensor (got {list(out.shape)})')
    plan = packed.passes(workspace_bytes)
    dev = out.device
    ts = stream_of(dev, stream)
    if packed.nshapes == 0:
        with torch.cuda.stream(ts):
            out.zero_()
        return
    need = _lib.lib().rmem_polygon_fill_workspace_bytes
    dc = packed.on_device(dev)
    ws = workspace('polygons.fill', dev, ts, max(int(need(p.plane_words)) for p in plan))
    dc.used_on(ts)
    out.record_stream(ts)
    from . import ops
    ops.copy_async(dc.bits[:packed.buf.numel()], packed.buf, packed.buf.numel())(ts.cuda_stream)
    for p in plan:
        fill_pass(packed, dc, p, ws, out, ts.cuda_stream)


def fill_label_stack(frames, size: Optional[Tuple[int, int]] = None, device=None) -> torch.Tensor:
    """uint8 [n, H, W] label maps on `device` of a clip's polygon annotations (what PackedPolygons takes, or a PackedPolygons):
    label[shape] = value per frame in listing order, 0 under no shape, under the even-odd rule at pixel centres (include/rmem.h;
    not pycocotools' frPoly: boundary pixels can differ from it).  One fill, then one synchronisation and one readback of the
    status words: a non-zero word raises RmemError naming the shape and the reasons."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RmemError('polygons.fill_label_stack: the target must be a GPU device (there is no host rasteriser)')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    packed = frames if isinstance(frames, PackedPolygons) else PackedPolygons(frames, size)
    stream = torch.cuda.current_stream(device)
    out = torch.empty(tuple(packed.shape), dtype=torch.uint8, device=device)
    fill_labels_into(packed, out, stream)
    if packed.nshapes:
        packed.check(device, 0, packed.nshapes, stream)
    return out
