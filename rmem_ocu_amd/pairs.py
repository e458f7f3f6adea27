"""Pair census: the overlap of every object of one label stack with every object of another, from one small table per frame.

rmem_clip_score_counts and rmem_mask_iou_counts compare predicted id i with annotated id i only.  Where the mask of a swapped
identity went, the spatio-temporal IoU of every predicted with every annotated track (YouTube-VIS / OVIS), the per-frame IoU
matrices association metrics start from (BURST / TAO-VOS) and the matching of predictions whose ids are not the annotation's are
all functions of the joint histogram of (predicted value, annotated value).  pair_census builds that table on the device
(rmem_label_pair_census, one call for the whole stack); pair_iou, track_iou and assign read it on the host after one readback.

The boundary half: pair_boundary_counts gives the boundary match counts of every pair (rmem_pair_boundary_counts), pair_f turns
them into the boundary accuracy F of every pair, pair_jf returns J and F of every pair -- what DAVIS's unsupervised matching and
clip scoring beyond 31 objects are built on (evaluator.score_unsupervised_clip, score_clip_objects).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import workspace
from ._labels import WORKSPACE_CAP as PAIR_BOUNDARY_WORKSPACE_CAP, boundary_prf, frames_per_pass, int_in, is_int, stack_pair
from ._lib import RmemError


def pair_census(a_u8: torch.Tensor, b_u8: torch.Tensor, num_a: int, num_b: int) -> torch.Tensor:
    """int32 [n, num_a + 2, num_b + 2] on the device: entry [f, i, j] counts the pixels of frame f with min(a, num_a + 1) == i and
    min(b, num_b + 1) == j (include/rmem.h, rmem_label_pair_census).  The last row and the last column are "other": every value
    above num_a / num_b, a void label of 255 included when num_b < 255.  Every frame's table sums to H * W.  a_u8, b_u8: uint8
    device stacks [n, H, W] or [H, W] of one shape on one device.  One call on the current stream, no host sync."""
    what = 'pairs.pair_census'
    num_a, num_b = int_in(what, 'num_a', num_a, 1, 255), int_in(what, 'num_b', num_b, 1, 255)
    a, b = stack_pair(what, a_u8, b_u8)
    n, H, W = a.shape
    out = torch.empty(n, num_a + 2, num_b + 2, dtype=torch.int32, device=a.device)
    stream = torch.cuda.current_stream(a.device)
    _lib.check(_lib.lib().rmem_label_pair_census(a.data_ptr(), b.data_ptr(), n, H, W, num_a, num_b, out.data_ptr(), stream.cuda_stream),
               'rmem_label_pair_census')
    for t in (a, b):
        t.record_stream(stream)
    return out


def _void(what: str, void_label, num_b: int) -> int:
    """the C entry points' void_label: -1 for None (no void), else an integer in num_b + 1 .. 255"""
    if void_label is None:
        return -1
    if not is_int(void_label) or not num_b < int(void_label) <= 255:
        raise RmemError(f'{what}: void_label must be None or an integer above num_b = {num_b}, at most 255 (got {void_label!r})')
    return int(void_label)


def pair_boundary_counts(a_u8: torch.Tensor, b_u8: torch.Tensor, num_a: int, num_b: int, void_label: Optional[int] = 255,
                         bound_th: float = 0.008, workspace_bytes: Optional[int] = None):
    """(match int32 [n, num_a + 1, num_b + 1, 2], bnd_a int32 [n, num_a + 1], bnd_b int32 [n, num_b + 1]) on the device: the
    boundary pixels of every object of a and of b, and for every pair (i, j) the boundary pixels of a's object i inside b's
    object j's boundary dilated by f_measure's disk ([..., 0]) and the other way round ([..., 1]) -- include/rmem.h,
    rmem_pair_boundary_counts.  Row and column 0 (background) are zero.  a_u8, b_u8: uint8 device stacks [n, H, W] or [H, W] of
    one shape on one device; pixels where b is void_label count on neither side; void_label None means no void (needed for
    num_b = 255).  bound_th: as evaluator.boundary_radius takes it.  One call on the current stream, no host sync.
    The bit planes live in a workspace per (device, stream) that holds as many frames as fit workspace_bytes (default: 256 MiB,
    or one frame's planes where those are larger); the call passes over the stack that many frames at a time."""
    what = 'pairs.pair_boundary_counts'
    num_a, num_b = int_in(what, 'num_a', num_a, 1, 255), int_in(what, 'num_b', num_b, 1, 255)
    void = _void(what, void_label, num_b)
    a, b = stack_pair(what, a_u8, b_u8)
    n, H, W = a.shape
    L = _lib.lib()
    radius = L.rmem_boundary_radius(H, W, float(bound_th))
    if not 1 <= radius <= 63:
        raise RmemError(f'{what}: the dilation radius must be in 1..63 (bound_th={bound_th} gives {radius} at {H} x {W})')
    per_frame = L.rmem_pair_boundary_workspace_bytes(1, H, W, num_a, num_b)
    if per_frame == 0:
        raise RmemError(f'{what}: frames of {H} x {W} are too large (H * W at most 2^26), or more than 65535 of them')
    nbytes = min(frames_per_pass(what, n, per_frame, workspace_bytes, 'one frame\'s planes')[0], n * per_frame)
    stream = torch.cuda.current_stream(a.device)
    ws = workspace('pair_boundary', a.device, stream, nbytes)
    match = torch.empty(n, num_a + 1, num_b + 1, 2, dtype=torch.int32, device=a.device)
    bnd_a = torch.empty(n, num_a + 1, dtype=torch.int32, device=a.device)
    bnd_b = torch.empty(n, num_b + 1, dtype=torch.int32, device=a.device)
    _lib.check(L.rmem_pair_boundary_counts(a.data_ptr(), b.data_ptr(), n, H, W, num_a, num_b, void, radius, ws.data_ptr(), nbytes,
                                           bnd_a.data_ptr(), bnd_b.data_ptr(), match.data_ptr(), stream.cuda_stream),
               'rmem_pair_boundary_counts')
    for t in (a, b):
        t.record_stream(stream)
    return match, bnd_a, bnd_b


def _host_ints(t, ndim: int, what: str, name: str) -> np.ndarray:
    c = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if c.ndim != ndim or not np.issubdtype(c.dtype, np.integer):
        raise RmemError(f'{what}: {name} must be an integer array of {ndim} dimensions (got {c.dtype} {c.shape})')
    return c


def pair_f(match, bnd_a, bnd_b) -> np.ndarray:
    """The boundary accuracy F of every pair, float64 [n, num_a, num_b], from pair_boundary_counts' three tables (device tensors:
    one readback each; or host arrays).  Entry [f, i - 1, j - 1] is object i of a against object j of b.  f_measure's edge cases
    are _labels.boundary_prf's, which evaluator.scores_from_counts calls as well."""
    what = 'pairs.pair_f'
    m, ba, bb = _host_ints(match, 4, what, 'match'), _host_ints(bnd_a, 2, what, 'bnd_a'), _host_ints(bnd_b, 2, what, 'bnd_b')
    if m.shape != (ba.shape[0], ba.shape[1], bb.shape[1], 2) or ba.shape[0] != bb.shape[0] or ba.shape[1] < 2 or bb.shape[1] < 2:
        raise RmemError(f'{what}: match [n, num_a + 1, num_b + 1, 2], bnd_a [n, num_a + 1] and bnd_b [n, num_b + 1] do not fit '
                        f'(got {m.shape}, {ba.shape}, {bb.shape})')
    fg_m, gt_m = m[:, 1:, 1:, 0].astype(np.float64), m[:, 1:, 1:, 1].astype(np.float64)
    n_fg = np.broadcast_to(ba[:, 1:, None], fg_m.shape).astype(np.float64)
    n_gt = np.broadcast_to(bb[:, None, 1:], fg_m.shape).astype(np.float64)
    return boundary_prf(n_fg, n_gt, fg_m, gt_m)[2]


def jf_from_tables(census, match, bnd_a, bnd_b, drop_other_b: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Host half of pair_jf: (J, F) float64 [n, num_a, num_b] from a pair census and pair_boundary_counts' tables (device tensors
    or host arrays).  J = pair_iou with db_eval_iou's "empty union is 1" on EVERY pair, as the benchmark toolkit scores a pair of
    empty masks; F = pair_f."""
    iou, _, union = pair_iou(census, drop_other_b=drop_other_b)
    F = pair_f(match, bnd_a, bnd_b)
    if iou.shape != F.shape:
        raise RmemError(f'pairs.jf_from_tables: the census is for {iou.shape[1:]} objects, the boundary tables for {F.shape[1:]}')
    return np.where(union == 0, 1.0, iou), F


def pair_jf(a_u8: torch.Tensor, b_u8: torch.Tensor, num_a: int, num_b: int, void_label: Optional[int] = 255,
            bound_th: float = 0.008) -> Tuple[np.ndarray, np.ndarray]:
    """(J, F) float64 [n, num_a, num_b]: the region similarity and the boundary accuracy of every object of a against every object
    of b on every frame (jf_from_tables).  With a void_label, annotated pixels of any value above num_b count nowhere in J
    (pair_iou's drop_other_b) and void pixels nowhere in F; without one every pixel counts.  Two device calls on the current
    stream (pair_census, pair_boundary_counts), then the readbacks."""
    census = pair_census(a_u8, b_u8, num_a, num_b)
    match, bnd_a, bnd_b = pair_boundary_counts(a_u8, b_u8, num_a, num_b, void_label, bound_th)
    return jf_from_tables(census, match, bnd_a, bnd_b, drop_other_b=void_label is not None)


def _table(census, what: str) -> np.ndarray:
    c = census.cpu().numpy() if isinstance(census, torch.Tensor) else np.asarray(census)
    if c.ndim != 3 or c.shape[1] < 3 or c.shape[2] < 3 or not np.issubdtype(c.dtype, np.integer):
        raise RmemError(f'{what}: census must be an integer [n, num_a + 2, num_b + 2] table (got {c.dtype} {c.shape})')
    return c.astype(np.int64)


def _inter_union(census, drop_other_b: bool, what: str) -> Tuple[np.ndarray, np.ndarray]:
    c = _table(census, what)
    num_a, num_b = c.shape[1] - 2, c.shape[2] - 2
    if drop_other_b:
        c = c[:, :, :-1]
    area_a, area_b = c.sum(axis=2), c.sum(axis=1)
    inter = c[:, 1:num_a + 1, 1:num_b + 1]
    union = area_a[:, 1:num_a + 1, None] + area_b[:, None, 1:num_b + 1] - inter
    return np.ascontiguousarray(inter), union


def pair_iou(census, drop_other_b: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(iou float64 [n, num_a, num_b], inter int64, union int64) of a pair census (a device tensor: one readback; or a host
    array).  Objects are 1..num: entry [f, i - 1, j - 1] is object i of a against object j of b on frame f, background is neither a
    row nor a column.  inter is the table's entry, union = area of a's object + area of b's object - inter with the areas summed
    over ALL rows and columns of the table.  drop_other_b removes b's "other" column first -- the void rule of
    rmem_mask_iou_counts: pixels whose annotation is void (or any value above num_b) count nowhere.  iou is NaN where the union is
    0: db_eval_iou's "empty union is 1" is the caller's to apply on the diagonal, off it every absent pair would be perfect."""
    inter, union = _inter_union(census, drop_other_b, 'pairs.pair_iou')
    iou = np.full(inter.shape, np.nan, dtype=np.float64)
    np.divide(inter, union, out=iou, where=union > 0)
    return iou, inter, union


def track_iou(census, frames=None, drop_other_b: bool = True) -> np.ndarray:
    """float64 [num_a, num_b]: sum over the chosen frames of the intersection over the sum of the union (both summed in int64), 0
    where the summed union is 0 -- the spatio-temporal IoU of every track of a with every track of b of YouTube-VIS-style
    evaluation.  frames: None (all), a slice or a sequence of frame indices."""
    inter, union = _inter_union(census, drop_other_b, 'pairs.track_iou')
    if frames is not None:
        sel = np.arange(inter.shape[0])[frames] if isinstance(frames, slice) else np.asarray(list(frames), dtype=np.int64)
        inter, union = inter[sel], union[sel]
    i, u = inter.sum(axis=0), union.sum(axis=0)
    out = np.zeros(i.shape, dtype=np.float64)
    np.divide(i, u, out=out, where=u > 0)
    return out


def _solve_square(cost: np.ndarray) -> Tuple[List[int], np.ndarray, np.ndarray]:
    """Minimum-cost perfect matching of a square matrix by shortest augmenting paths (the Hungarian method with potentials,
    O(N^3), the inner loop in numpy) -> (column of every row, row potentials u, column potentials v) with u[i] + v[j] <= cost[i, j]
    everywhere and equality on the matching."""
    N = cost.shape[0]
    u, v = np.zeros(N + 1), np.zeros(N + 1)
    p = np.zeros(N + 1, dtype=np.int64)                            # p[j]: the row (1-based) matched to column j, 0 = free
    way = np.zeros(N + 1, dtype=np.int64)
    a = np.zeros((N + 1, N + 1))
    a[1:, 1:] = cost
    for i in range(1, N + 1):
        p[0] = i
        j0 = 0
        minv = np.full(N + 1, np.inf)
        used = np.zeros(N + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = a[i0] - u[i0] - v
            better = ~used & (cur < minv)
            better[0] = False
            minv[better] = cur[better]
            way[better] = j0
            free = np.where(used, np.inf, minv)
            free[0] = np.inf
            j1 = int(np.argmin(free))
            delta = free[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = int(way[j0])
            p[j0] = p[j1]
            j0 = j1
    col = [0] * N
    for j in range(1, N + 1):
        col[int(p[j]) - 1] = j - 1
    return col, u[1:], v[1:]


def _smallest_matching(col: List[int], tight: np.ndarray, rows: int) -> List[int]:
    """The lexicographically smallest perfect matching of the bipartite graph `tight` (N x N, bool), starting from the perfect
    matching `col`: rows in ascending order take the smallest column that still leaves the rows after them a perfect matching."""
    N = len(col)
    adj = [np.nonzero(tight[i])[0].tolist() for i in range(N)]
    row_of = [0] * N
    for i, j in enumerate(col):
        row_of[j] = i
    fixed = [False] * N                                            # columns of the rows already decided
    for i in range(rows):
        cur = col[i]
        for j in adj[i]:
            if j >= cur:
                break
            if fixed[j]:
                continue
            # row i takes j: the row that holds j needs a way to cur through rows after i, over tight edges
            start = row_of[j]
            parent = {start: None}                                 # row -> (previous row, the column taken from it)
            queue, end = [start], None
            while queue and end is None:
                r = queue.pop()
                for c in adj[r]:
                    if c == cur:
                        end = r
                        break
                    if fixed[c] or c == j:
                        continue
                    nxt = row_of[c]
                    if nxt not in parent:
                        parent[nxt] = (r, c)
                        queue.append(nxt)
            if end is None:
                continue
            r, c = end, cur
            while r is not None:                                   # shift the columns along the path
                step = parent[r]
                col[r], row_of[c] = c, r
                if step is None:
                    break
                r, c = step[0], step[1]
            col[i], row_of[j] = j, i
            break
        fixed[col[i]] = True
    return col


def assign(score, minimum: float = 0.0) -> List[Tuple[int, int]]:
    """The one-to-one assignment of rows to columns with the largest total score, as a list of (row, column) in ascending rows.
    score: a finite [R, C] matrix, 1 <= R, C <= 255 (track_iou's result).  min(R, C) pairs are chosen -- every row when R <= C,
    every column otherwise -- and among the choices of equal total the lexicographically smallest list is taken, so the result is
    reproducible; then the pairs whose score is not above `minimum` are left out.  Totals are equal when they differ by rounding
    only: the tie rule looks at edges whose reduced cost is within 1e-12 of the largest |score|.
    The Hungarian method in numpy, O(max(R, C)^3), followed by the tie rule on the tight edges (one augmenting-path search per
    edge it rejects)."""
    s = np.asarray(score, dtype=np.float64)
    if s.ndim != 2 or not 1 <= s.shape[0] <= 255 or not 1 <= s.shape[1] <= 255:
        raise RmemError(f'pairs.assign: score must be a [R, C] matrix with 1 <= R, C <= 255 (got {s.shape})')
    if not np.isfinite(s).all():
        raise RmemError('pairs.assign: score must be finite (pair_iou marks an empty union with NaN: use track_iou, or fill it in)')
    R, Cn = s.shape
    N = max(R, Cn)
    cost = np.zeros((N, N))                                        # rows / columns beyond the matrix: free for everyone
    cost[:R, :Cn] = -s
    col, u, v = _solve_square(cost)
    tol = 1e-12 * max(float(np.abs(s).max()), 1.0)
    tight = cost - u[:, None] - v[None, :] <= tol
    col = _smallest_matching(col, tight, R)
    return [(i, col[i]) for i in range(R) if col[i] < Cn and s[i, col[i]] > minimum]
