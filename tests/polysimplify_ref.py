"""Sequential restatement of the ring simplification contract of include/rmem.h (rmem_polygon_simplify) with Python integers
and an explicit stack, written from the contract and never from the kernels.  The package does not import it.  Also the far-pixel
mask of the fill-back property, an exact rational distance that shares nothing with the rule's keys, the rings the device tests
aim at the kernels (teeth of growing height: a recursion as deep as the ring is long) and the contents they trace."""
from fractions import Fraction

import numpy as np

import census_ref
import polygons_ref as P

ST_TABLE, ST_RING = 8, 16
MAX_COORD = 32767


def steps(tolerance):
    """T of a tolerance in pixels: 1/16 pixel steps"""
    return int(np.rint(16.0 * float(tolerance)))


def key_thr(pi, pj, pm, T):
    """(key, thr) of vertex pm against the segment pi pj"""
    ax, ay, bx, by = pj[0] - pi[0], pj[1] - pi[1], pm[0] - pi[0], pm[1] - pi[1]
    L, bb, t = ax * ax + ay * ay, bx * bx + by * by, ax * bx + ay * by
    if L == 0:
        return bb, (T * T) // 256
    thr = (T * T * L) // 256
    if t <= 0:
        return bb * L, thr
    if t >= L:
        return ((pm[0] - pj[0]) ** 2 + (pm[1] - pj[1]) ** 2) * L, thr
    return (ax * by - ay * bx) ** 2, thr


def simplify_ring(pts, T, with_depth=False):
    """the sorted indices the rule keeps of a ring [(x, y), ...], k >= 1 (and the depth the recursion reached)"""
    p = [(int(x), int(y)) for x, y in pts]
    k = len(p)
    assert k >= 1
    if k == 1:
        return ([0], 0) if with_depth else [0]
    d2 = [(p[m][0] - p[0][0]) ** 2 + (p[m][1] - p[0][1]) ** 2 for m in range(k)]
    B = max(range(1, k), key=lambda m: (d2[m], -m))
    kept = {0, B}
    todo, deepest = [(0, B, 1), (B, k, 1)], 0
    while todo:
        i, j, depth = todo.pop()
        if j - i < 2:
            continue
        deepest = max(deepest, depth)
        pj = p[j % k]                                               # p_k := p_0
        best, at, thr = -1, -1, 0
        for m in range(i + 1, j):
            key, thr = key_thr(p[i], pj, p[m], T)
            if key > best:                                          # strictly: the smallest m among equals
                best, at = key, m
        if best > thr:
            kept.add(at)
            todo += [(i, at, depth + 1), (at, j, depth + 1)]
    return (sorted(kept), deepest) if with_depth else sorted(kept)


def simplify_arrays(rings, verts, counts, T, max_rings=None, max_verts=None):
    """(rings_out [R, 8], verts_out [V_out, 2], counts_out [4]) as rmem_polygon_simplify writes them: the used rows only"""
    rings, verts = np.asarray(rings).reshape(-1, 8), np.asarray(verts).reshape(-1, 2)
    max_rings = len(rings) if max_rings is None else max_rings
    max_verts = len(verts) if max_verts is None else max_verts
    _, R, V, status = (int(c) for c in counts)
    none = (np.zeros((0, 8), dtype=np.int32), np.zeros((0, 2), dtype=np.int32))
    if status:
        return none + (np.array([V, 0, 0, status], dtype=np.int32),)
    good = [0 <= int(r[2]) and int(r[3]) >= 1 and int(r[2]) + int(r[3]) <= V for r in rings[:max(R, 0)]] if 0 <= R <= max_rings else []
    if not (0 <= R <= max_rings and 0 <= V <= max_verts) or sum(int(r[3]) for r, g in zip(rings, good) if g) > max_verts:
        return none + (np.array([V, 0, 0, ST_TABLE], dtype=np.int32),)
    rows, out = [], []
    at = 0
    for r, g in zip(rings[:R], good):
        row = [int(v) for v in r]
        mine = verts[row[2]:row[2] + row[3]] if g else verts[:0]
        if not g or mine.min() < 0 or mine.max() > MAX_COORD:
            status |= ST_RING
            keep = []
        else:
            keep = simplify_ring(mine.tolist(), T)
        rows.append(row[:2] + [at, len(keep)] + row[4:7] + [row[3]])
        out.append(mine[keep])
        at += len(keep)
    rings_out = np.array(rows, dtype=np.int32).reshape(-1, 8)
    verts_out = np.concatenate(out).astype(np.int32) if out else none[1]
    return rings_out, verts_out.reshape(-1, 2), np.array([V, R, at, status], dtype=np.int32)


def within(pi, pj, pm, tolerance):
    """pm is within `tolerance` (a Fraction) of the segment pi pj, in exact rationals: the nearest point by projection, clamped"""
    ax, ay = pj[0] - pi[0], pj[1] - pi[1]
    L = ax * ax + ay * ay
    s = Fraction(0) if L == 0 else min(max(Fraction(ax * (pm[0] - pi[0]) + ay * (pm[1] - pi[1]), L), Fraction(0)), Fraction(1))
    dx, dy = pi[0] + s * ax - pm[0], pi[1] + s * ay - pm[1]
    return dx * dx + dy * dy <= tolerance * tolerance


def far_pixels(stack, num_objs, tolerance):
    """bool [n, H, W]: the pixels whose (2r + 1)^2 window, r = ceil(tolerance) + 1, holds one object value only.  Values above
    num_objs count as 0; the frame is padded with a value that is no object -- a ring edge runs along the frame's border wherever
    an object touches it, so a window that leaves the frame is never far."""
    a = np.asarray(stack).astype(np.int64)
    a = np.where(a > num_objs, 0, a)
    n, H, W = a.shape
    r = int(np.ceil(tolerance)) + 1
    pad = np.full((n, H + 2 * r, W + 2 * r), -1, dtype=np.int64)
    pad[:, r:r + H, r:r + W] = a
    far = np.ones((n, H, W), dtype=bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            far &= pad[:, dy:dy + H, dx:dx + W] == a
    return far


def shapes(rings, verts, n, num_objs):
    """polyfill_ref.paint_stack's frames of a ring table: the objects of a frame in value order, each one even-odd shape of all
    its rings that have a vertex"""
    frames = [[(v, []) for v in range(1, num_objs + 1)] for _ in range(n)]
    for r in np.asarray(rings).reshape(-1, 8):
        if 1 <= r[1] <= num_objs and r[3] >= 1:
            frames[r[0]][r[1] - 1][1].append(np.asarray(verts)[r[2]:r[2] + r[3]])
    return [[(v, rs) for v, rs in fr if rs] for fr in frames]


# ------------------------------------------------------------------------------------------------------------- rings and contents
def teeth(k, pad=0):
    """a ring of 2 k + 3 + pad vertices: k teeth of strictly growing height on a base line, closed below (`pad` more vertices
    on the closing edge).  The rule peels it a tooth at a time: its recursion is about 2 k deep."""
    assert k >= 1 and 0 <= pad < 2 * k
    v = []
    for i in range(k):
        v += [(2 * i, 1), (2 * i + 1, 2 + i)]
    v += [(2 * k, 1), (2 * k, 0)] + [(2 * k - j, 0) for j in range(1, pad + 1)] + [(0, 0)]
    return np.array(v, dtype=np.int32)


def table(ring_list, frame=0, value=1):
    """(rings [R, 8], verts [V, 2], counts [4]) of hand-made rings, laid out as the tracer does"""
    rows, at = [], 0
    for k, r in enumerate(ring_list):
        rows.append([frame, value, at, len(r), 0, 4 * k, len(r), 0])
        at += len(r)
    verts = np.concatenate([np.asarray(r, dtype=np.int32).reshape(-1, 2) for r in ring_list])
    return np.array(rows, dtype=np.int32).reshape(-1, 8), verts, np.array([at, len(rows), at, 0], dtype=np.int32)


def smooth_blobs(seed, n, H, W, objects=3):
    """`objects` overlapping ellipses with wavy outlines on background 0, drifting from frame to frame: smooth, large pieces"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.zeros((n, H, W), dtype=np.uint8)
    for v in range(1, objects + 1):
        cy, cx = rng.uniform(0.25, 0.75) * H, rng.uniform(0.25, 0.75) * W
        ry, rx = rng.uniform(0.18, 0.3) * H, rng.uniform(0.18, 0.3) * W
        lobes, phase = int(rng.integers(2, 5)), rng.uniform(0, 2 * np.pi)
        for f in range(n):
            dy, dx = yy - (cy + f), xx - (cx + 2 * f)
            wave = 1.0 + 0.15 * np.cos(lobes * np.arctan2(dy, dx) + phase)
            a[f][(dy / ry) ** 2 + (dx / rx) ** 2 <= wave * wave] = v
    return a


CONTENTS = ('zero', 'full', 'blobs', 'speckle', 'noise', 'checker', 'stripes', 'serpentine', 'concentric', 'nest', 'others')


def content(name, shape, num_objs=10):
    """the contents of the tracer's tests, from polygons_ref and census_ref"""
    n, H, W = shape
    seed = n * 7919 + H * 131 + W
    if name == 'zero':
        a = np.zeros(shape, dtype=np.uint8)
    elif name == 'full':
        a = np.full(shape, 3, dtype=np.uint8)
    elif name == 'blobs':
        a = smooth_blobs(seed, n, H, W)
    elif name == 'speckle':
        a = P.speckle(census_ref.blobs(seed, n, H, W), seed, 0.01, num_objs)
    elif name == 'noise':
        a = P.noise(seed, n, H, W, 4)
    elif name == 'checker':
        a = P.checkerboard(n, H, W)
    elif name == 'stripes':
        a = P.stripes(n, H, W)
    elif name == 'serpentine':
        a = P.serpentine(n, H, W)
    elif name == 'concentric':
        a = P.concentric(n, H, W)
    elif name == 'nest':
        a = P.nest(n, H, W)
    else:
        assert name == 'others'
        a = P.with_other_values(census_ref.blobs(seed, n, H, W), num_objs, seed)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.shape == tuple(shape)
    return a
