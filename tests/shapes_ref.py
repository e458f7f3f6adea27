"""numpy / Python-int restatement of the shape census (include/rmem.h, rmem_label_moments and the hull entry points;
rmem_ocu_amd.shapes), written independently of it: brute-force moments (numpy int64 sums, exact below 2^63), row extents, the convex hull as a monotone chain over ALL
unique pixel corners of a mask (no use of the row-extent idea), the exact minimum-area rectangle by Fraction, and the float
properties from the same closed forms.  Further down, the two restatements of the DEVICE method the host tests compare with the
brute force (levels from row extents: the serial chain and the O(h^2) membership rule), and the contents the tests share."""
import math
from fractions import Fraction

import numpy as np


def moments(labels):
    """int64 [n, 256, 6] = (m00, m10, m01, m20, m11, m02) per frame and value: every sum is below 2^55, so int64 sums are exact"""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    out = np.zeros((n, 256, 6), dtype=np.int64)
    for f in range(n):
        for v in np.unique(labels[f]):
            ys, xs = np.nonzero(labels[f] == v)
            x, y = xs.astype(np.int64), ys.astype(np.int64)
            out[f, int(v)] = (x.size, x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum())
    return out


def uniform_moments(H, W):
    """the six sums of a frame filled with one value, closed forms in Python ints"""
    sx, sy = W * (W - 1) // 2, H * (H - 1) // 2
    sxx, syy = (W - 1) * W * (2 * W - 1) // 6, (H - 1) * H * (2 * H - 1) // 6
    return (H * W, H * sx, W * sy, H * sxx, sx * sy, W * syy)


def extents(labels, num):
    """int32 [n, num, H, 2] = (xmin, xmax) of value v = 1..num on row y, (W, -1) where the row lacks it"""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    out = np.empty((n, num, H, 2), dtype=np.int32)
    out[..., 0], out[..., 1] = W, -1
    for f in range(n):
        for v in range(1, num + 1):
            for y in range(H):
                xs = np.nonzero(labels[f, y] == v)[0]
                if xs.size:
                    out[f, v - 1, y] = (xs[0], xs[-1])
    return out


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def canonical(ring):
    """a strictly convex ring of (x, y) in either direction -> int32 [k, 2] starting at the smallest (y, x), shoelace sum positive"""
    pts = [(int(x), int(y)) for x, y in ring]
    if len(pts) >= 3 and area2(pts) < 0:
        pts.reverse()
    s = min(range(len(pts)), key=lambda i: (pts[i][1], pts[i][0]))
    return np.array(pts[s:] + pts[:s], dtype=np.int32).reshape(-1, 2)


def area2(ring):
    p = [(int(x), int(y)) for x, y in ring]
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(p, p[1:] + p[:1]))


def hull(mask):
    """convex hull of the pixel squares of a 2-D bool mask: Andrew's monotone chain over every unique corner, collinear points
    dropped, canonical; int32 [0, 2] for an empty mask"""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return np.zeros((0, 2), dtype=np.int32)
    side = int(ys.max()) + 2                                       # every unique corner, in (x, y) order, through one sorted key
    keys = np.unique(np.concatenate([(xs + dx).astype(np.int64) * side + (ys + dy) for dx in (0, 1) for dy in (0, 1)]))
    pts = list(zip((keys // side).tolist(), (keys % side).tolist()))
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return canonical(lower[:-1] + upper[:-1])


def hulls(labels, num):
    """(verts int32 [V, 2], offsets int32 [n * num + 1]) of the stack: ring after ring, empty ranges for absent objects"""
    labels = np.asarray(labels)
    rings = [hull(labels[f] == v) for f in range(labels.shape[0]) for v in range(1, num + 1)]
    off = np.zeros(len(rings) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rings])
    verts = np.concatenate(rings).astype(np.int32) if rings else np.zeros((0, 2), dtype=np.int32)
    return verts.reshape(-1, 2), off


def min_rect(ring):
    """(area Fraction, index of the edge it lies on, corners float64 [4, 2]) of the minimum-area enclosing rectangle of a convex
    ring: every edge tried, areas compared as Fractions, the first edge in ring order on a tie"""
    p = [(int(x), int(y)) for x, y in ring]
    best = None
    for i in range(len(p)):
        (x0, y0), (x1, y1) = p[i], p[(i + 1) % len(p)]
        ex, ey = x1 - x0, y1 - y0
        dots = [q[0] * ex + q[1] * ey for q in p]
        crosses = [ex * q[1] - ey * q[0] for q in p]
        a = Fraction((max(dots) - min(dots)) * (max(crosses) - min(crosses)), ex * ex + ey * ey)
        if best is None or a < best[0]:
            best = (a, i, (ex, ey, min(dots), max(dots), min(crosses), max(crosses)))
    a, i, (ex, ey, d0, d1, c0, c1) = best
    e2 = ex * ex + ey * ey
    # the point with p.e = d and e x p = c is (d e + c n) / |e|^2 with n = (-ey, ex)
    corners = np.array([[(d * ex - c * ey) / e2, (d * ey + c * ex) / e2] for d, c in ((d0, c0), (d1, c0), (d1, c1), (d0, c1))], dtype=np.float64)
    return a, i, corners


def feret2(ring):
    p = [(int(x), int(y)) for x, y in ring]
    return max((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 for a in p for b in p)


def props(mask):
    """the dict of shapes.props_from_tables for one 2-D bool mask (not empty), from the brute-force parts above"""
    ys, xs = np.nonzero(np.asarray(mask))
    x, y = [int(t) for t in xs], [int(t) for t in ys]
    m00, m10, m01 = len(x), sum(x), sum(y)
    m20, m11, m02 = sum(t * t for t in x), sum(a * b for a, b in zip(x, y)), sum(t * t for t in y)
    mu = (m00 * m20 - m10 * m10, m00 * m11 - m10 * m01, m00 * m02 - m01 * m01)
    u20, u11, u02 = (t / (m00 * m00) for t in mu)
    root = math.sqrt((u20 - u02) ** 2 + 4.0 * u11 * u11)
    l1, l2 = (u20 + u02 + root) / 2.0, max((u20 + u02 - root) / 2.0, 0.0)
    ring = hull(mask)
    h2 = area2(ring)
    a, _, corners = min_rect(ring)
    return dict(area=m00, centroid=(m10 / m00, m01 / m00), mu=mu,
                orientation=0.0 if mu[1] == 0 and mu[0] == mu[2] else 0.5 * math.atan2(2 * mu[1], mu[0] - mu[2]),
                major_axis=4.0 * math.sqrt(l1), minor_axis=4.0 * math.sqrt(l2),
                eccentricity=0.0 if l1 == 0 else math.sqrt(max(1.0 - l2 / l1, 0.0)),
                hull=ring, hull_area2=h2, solidity=2 * m00 / h2,
                extent=m00 / ((max(x) - min(x) + 1) * (max(y) - min(y) + 1)),
                feret2=feret2(ring), min_rect=corners, min_rect_area=a.numerator / a.denominator)


def stack_props(labels, num, squeeze_idx=None):
    """[{key: props} per frame] for the objects 1..num, absent ones left out; keys as _labels.object_keys gives them"""
    labels = np.asarray(labels)
    out = []
    for f in range(labels.shape[0]):
        fr = {}
        for v in range(1, num + 1):
            if squeeze_idx is not None and v >= len(squeeze_idx):
                continue
            m = labels[f] == v
            if m.any():
                fr[v if squeeze_idx is None else int(squeeze_idx[v])] = props(m)
        out.append(fr)
    return out


# --------------------------------------------------------------------------------------------- the device method, restated
def levels(ext_rows, W):
    """(L, R) int lists over the corner levels 0..H of one object's extents [H, 2]; None where a level has no candidate"""
    H = len(ext_rows)
    L, R = [None] * (H + 1), [None] * (H + 1)
    for l in range(H + 1):
        rows = [ext_rows[y] for y in (l - 1, l) if 0 <= y < H and ext_rows[y][1] >= 0]
        if rows:
            L[l], R[l] = min(int(r[0]) for r in rows), max(int(r[1]) for r in rows) + 1
    return L, R


def _ring_from_chains(L, R, left, right):
    """the canonical ring of the vertex levels of both chains (ascending): (L, top), down the right chain, up the left chain"""
    if not left:
        return np.zeros((0, 2), dtype=np.int32)
    ring = [(L[left[0]], left[0])] + [(R[l], l) for l in right] + [(L[l], l) for l in reversed(left[1:])]
    return np.array(ring, dtype=np.int32).reshape(-1, 2)


def hull_by_level_chains(ext_rows, W):
    """the serial form: a monotone-chain stack walk over the levels, once for L (convex minorant) and once for R (majorant)"""
    L, R = levels(ext_rows, W)

    def chain(vals, sign):
        st = []
        for l, v in enumerate(vals):
            if v is None:
                continue
            while len(st) >= 2 and sign * ((st[-1][0] - st[-2][0]) * (v - st[-1][1]) - (st[-1][1] - st[-2][1]) * (l - st[-1][0])) <= 0:
                st.pop()
            st.append((l, v))
        return [l for l, _ in st]
    return _ring_from_chains(L, R, chain(L, 1), chain(R, -1))


def hull_by_level_membership(ext_rows, W):
    """the parallel form: level i is a vertex iff it is an end level or turns strictly against EVERY pair j < i < k"""
    L, R = levels(ext_rows, W)
    cand = [l for l, v in enumerate(L) if v is not None]

    def members(vals, sign):
        out = []
        for i in cand:
            if i in (cand[0], cand[-1]) or all(sign * ((i - j) * (vals[k] - vals[i]) - (vals[i] - vals[j]) * (k - i)) > 0
                                               for j in cand if j < i for k in cand if k > i):
                out.append(i)
        return out
    return _ring_from_chains(L, R, members(L, 1), members(R, -1)) if cand else np.zeros((0, 2), dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- contents
def disc(H, W, cy, cx, r):
    y, x = np.mgrid[:H, :W]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r
