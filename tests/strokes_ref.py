"""The stroke rasteriser's contract (include/rmem.h, rmem_stroke_draw_labels), restated sequentially in Python integers, so it is
exact at any size.  Pixel-index coordinates: the centre of pixel (y, x) is the point (x, y); fixed point is 1/256 pixel,
X = rint(256 x) in float64 (ties to even); pixel (py, px) is P = (256 px, 256 py).

Round brush, R >= 1: a stroke covers the pixels whose centre lies within R of any of its segments (a lone point: the segment
A -> A).  For A -> B with d = B - A, w = P - A, t = w.d, L = d.d: t <= 0: |w|^2 <= R^2; t >= L: |P - B|^2 <= R^2; otherwise
(w x d)^2 <= R^2 L.
Hairline, R == 0: per segment, oriented along its major axis M (x if |dX| >= |dY|, else y) so that dM > 0, the pixel of each
endpoint rounded half up per axis, (X + 128) >> 8, and for every integer k with A_M <= 256 k <= B_M the pixel with major index k
and minor index floor((N + 128 dM) / (256 dM)), N = A_m dM + (256 k - A_M) d_m.  A segment with d = 0 draws its endpoint's pixel.
A frame paints its strokes in listing order, the later one wins, 0 under none or the byte of `base`.  Off the frame is clipped.

Nothing here is shared with rmem_ocu_amd/strokes.py: the pack is checked against a direct count in test_strokes_host.py."""
import math

import numpy as np

FIXED = 256


def quantise(v):
    """rint(256 v) in float64, ties to even, as a Python int"""
    return int(np.rint(np.float64(v) * FIXED))


def points(path, origin='centre'):
    """[(X, Y), ...] of a path [[x, y], ...] or flat, consecutive repeats dropped"""
    a = np.asarray(path, dtype=np.float64).reshape(-1, 2)
    off = 0.5 if origin == 'corner' else 0.0
    out = []
    for x, y in a:
        q = (quantise(x - off), quantise(y - off))
        if not out or out[-1] != q:
            out.append(q)
    return out


def segments(pts):
    return [(pts[0], pts[0])] if len(pts) == 1 else list(zip(pts, pts[1:]))


def brush_covers(P, A, B, R):
    """the round-brush rule for one pixel centre and one segment, all in 1/256 pixel"""
    dx, dy = B[0] - A[0], B[1] - A[1]
    wx, wy = P[0] - A[0], P[1] - A[1]
    t, L = wx * dx + wy * dy, dx * dx + dy * dy
    if t <= 0:
        return wx * wx + wy * wy <= R * R
    if t >= L:
        ux, uy = P[0] - B[0], P[1] - B[1]
        return ux * ux + uy * uy <= R * R
    c = wx * dy - wy * dx
    return c * c <= R * R * L


def brush_pixels(pts, R, H, W):
    """{(y, x)} of a round-brush stroke inside the frame: every pixel of every segment's box against the rule"""
    out = set()
    for A, B in segments(pts):
        x0 = max(0, -((R - min(A[0], B[0])) // FIXED))
        x1 = min(W - 1, (max(A[0], B[0]) + R) // FIXED)
        y0 = max(0, -((R - min(A[1], B[1])) // FIXED))
        y1 = min(H - 1, (max(A[1], B[1]) + R) // FIXED)
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                if (y, x) not in out and brush_covers((FIXED * x, FIXED * y), A, B, R):
                    out.add((y, x))
    return out


def hairline_pixels(pts, H, W):
    """{(y, x)} of a hairline stroke inside the frame"""
    out = set()

    def put(x, y):
        if 0 <= x < W and 0 <= y < H:
            out.add((y, x))

    for A, B in segments(pts):
        put((A[0] + 128) >> 8, (A[1] + 128) >> 8)
        put((B[0] + 128) >> 8, (B[1] + 128) >> 8)
        if A == B:
            continue
        M = 0 if abs(B[0] - A[0]) >= abs(B[1] - A[1]) else 1
        m = 1 - M
        if B[M] < A[M]:
            A, B = B, A
        dM, dm = B[M] - A[M], B[m] - A[m]
        top = (W, H)[M]
        for k in range(max(0, -((-A[M]) // FIXED)), min(top - 1, B[M] // FIXED) + 1):
            N = A[m] * dM + (FIXED * k - A[M]) * dm
            n = (N + 128 * dM) // (FIXED * dM)
            put(*((k, n) if M == 0 else (n, k)))
    return out


def stroke_parts(stroke):
    """(value, path, radius) of a stroke dict or tuple"""
    if isinstance(stroke, dict):
        return stroke['value'], stroke['path'], stroke.get('radius', 0)
    return stroke[0], stroke[1], (stroke[2] if len(stroke) > 2 else 0)


def stroke_pixels(path, radius, H, W, origin='centre'):
    R = quantise(radius)
    pts = points(path, origin)
    return hairline_pixels(pts, H, W) if R == 0 else brush_pixels(pts, R, H, W)


def stroke_sets(frames, H, W, origin='centre'):
    """[[(value, {(y, x)}), ...] per frame]: every stroke's pixels, computed once, for painting in any order"""
    return [[(stroke_parts(s)[0], stroke_pixels(stroke_parts(s)[1], stroke_parts(s)[2], H, W, origin)) for s in strokes] for strokes in frames]


def paint_sets(sets, H, W, base=None):
    """uint8 [n, H, W] of stroke_sets' output in painting order, over zeros or over a copy of base"""
    out = np.zeros((len(sets), H, W), dtype=np.uint8) if base is None else np.array(base, dtype=np.uint8, copy=True)
    for f, strokes in enumerate(sets):
        for value, pixels in strokes:
            for y, x in pixels:
                out[f, y, x] = value
    return out


def paint_stack(frames, H, W, base=None, origin='centre'):
    """uint8 [n, H, W]: frames[f] = [stroke, ...] in painting order, over zeros or over a copy of base"""
    return paint_sets(stroke_sets(frames, H, W, origin), H, W, base)


def brush_mask_large(pts, R, H, W):
    """bool [H, W] of a round-brush stroke, for frames too large for brush_pixels: the same rule on whole int64 arrays (every term
    stays below 2^60), the 128-bit comparison c^2 <= R^2 L taken as |c| <= isqrt(R^2 L), which is the same for an integer c"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64) * FIXED
    out = np.zeros((H, W), dtype=bool)
    for A, B in segments(pts):
        dx, dy = B[0] - A[0], B[1] - A[1]
        wx, wy = xs - A[0], ys - A[1]
        t, L = wx * dx + wy * dy, dx * dx + dy * dy
        near_a = wx * wx + wy * wy <= R * R
        near_b = (xs - B[0]) ** 2 + (ys - B[1]) ** 2 <= R * R
        side = np.abs(wx * dy - wy * dx) <= math.isqrt(R * R * L)
        out |= np.where(t <= 0, near_a, np.where(t >= L, near_b, side))
    return out


def mask_of(pixels, H, W):
    m = np.zeros((H, W), dtype=bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def float_distance(path, H, W):
    """float64 [H, W]: the distance of every pixel centre to the polyline, brute force over the UNQUANTISED points"""
    a = np.asarray(path, dtype=np.float64).reshape(-1, 2)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    best = np.full((H, W), np.inf)
    pairs = [(a[0], a[0])] if len(a) == 1 else list(zip(a[:-1], a[1:]))
    for p, q in pairs:
        d = q - p
        L = float(d @ d)
        t = np.zeros((H, W)) if L == 0 else np.clip(((xs - p[0]) * d[0] + (ys - p[1]) * d[1]) / L, 0.0, 1.0)
        best = np.minimum(best, np.hypot(xs - (p[0] + t * d[0]), ys - (p[1] + t * d[1])))
    return best


def components8(pixels):
    """the number of 8-connected pieces of a set of (y, x), by flood fill"""
    left, pieces = set(pixels), 0
    while left:
        pieces += 1
        todo = [left.pop()]
        while todo:
            y, x = todo.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = (y + dy, x + dx)
                    if q in left:
                        left.remove(q)
                        todo.append(q)
    return pieces


# ---------------------------------------------------------------------------------------------------------------- generators
def random_walk(rng, H, W, k, step=None, margin=0.0, grid=None):
    """a polyline of k points: a random walk that starts anywhere within `margin` pixels around the frame; grid: the points are
    multiples of it (1/256 pixel is exact in float64, so the float test sees what the quantiser sees)"""
    step = max(H, W) / 6.0 if step is None else step
    p = np.array([rng.uniform(-margin, W - 1 + margin), rng.uniform(-margin, H - 1 + margin)])
    out = [p]
    for _ in range(k - 1):
        p = p + rng.uniform(-step, step, size=2)
        out.append(p)
    a = np.array(out)
    if grid:
        a = np.rint(a / grid) * grid
    return a


def random_strokes(seed, H, W, count, radii=(0, 0.4, 1, 2.5, 7), k=6, step=None):
    """`count` strokes for one frame: values 1..255 with an eraser now and then, radii in turn, some paths leaving the frame"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        value = 0 if i % 11 == 7 else 1 + int(rng.integers(0, 255))
        pts = random_walk(rng, H, W, 1 if i % 5 == 3 else 2 + int(rng.integers(0, k)), step=step, margin=3.0)
        out.append({'value': value, 'path': pts, 'radius': radii[i % len(radii)]})
    return out


def neighbour_path(rng, H, W, k):
    """k distinct-step pixels (x, y), each an 8-neighbour of the one before, inside the frame"""
    x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
    out = [(x, y)]
    while len(out) < k:
        dx, dy = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
        if (dx or dy) and 0 <= x + dx < W and 0 <= y + dy < H:
            x, y = x + dx, y + dy
            out.append((x, y))
        elif H == 1 and W == 1:
            break
    return out


def tie_cases():
    """[(name, stroke, H, W, the pixels wanted {(y, x)})]: ties at exactly half a pixel, vertices on centres and corners"""
    return [
        ('hairline endpoints at half pixels round half up', {'value': 1, 'path': [(1.5, 2.5)], 'radius': 0}, 6, 6, {(3, 2)}),
        ('a horizontal hairline at y + 0.5 goes down', {'value': 1, 'path': [(0, 1.5), (3, 1.5)], 'radius': 0}, 4, 5, {(2, 0), (2, 1), (2, 2), (2, 3)}),
        ('a vertical hairline at x - 0.5 rounds half up', {'value': 1, 'path': [(-0.5, 0), (-0.5, 2)], 'radius': 0}, 4, 4, {(0, 0), (1, 0), (2, 0)}),
        ('a slope-1/2 hairline: the minor coordinate ties at every other sample', {'value': 1, 'path': [(0, 0), (4, 2)], 'radius': 0}, 4, 6,
         {(0, 0), (1, 1), (1, 2), (2, 3), (2, 4)}),
        ('the reversed slope-1/2 hairline', {'value': 1, 'path': [(4, 2), (0, 0)], 'radius': 0}, 4, 6, {(0, 0), (1, 1), (1, 2), (2, 3), (2, 4)}),
        ('a disc of radius 1 on a centre holds its 4-neighbours', {'value': 1, 'path': [(2, 2)], 'radius': 1}, 5, 5,
         {(2, 2), (1, 2), (3, 2), (2, 1), (2, 3)}),
        ('a disc of radius sqrt(1/2) rounded down on a corner holds nothing', {'value': 1, 'path': [(1.5, 1.5)], 'radius': 181 / 256}, 4, 4, set()),
        ('a disc of radius sqrt(1/2) rounded up on a corner holds its four pixels', {'value': 1, 'path': [(1.5, 1.5)], 'radius': 182 / 256}, 4, 4,
         {(1, 1), (1, 2), (2, 1), (2, 2)}),
        ('a brush of half a pixel along a row boundary holds both rows', {'value': 1, 'path': [(1, 1.5), (3, 1.5)], 'radius': 0.5}, 4, 5,
         {(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)}),
        ('a brush of exactly the distance: the side is inclusive', {'value': 1, 'path': [(0, 0), (4, 0)], 'radius': 2}, 4, 5,
         {(y, x) for y in range(3) for x in range(5)} | {(0, 0)}),
    ]
