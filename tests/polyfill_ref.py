"""Sequential restatement of the polygon fill contract of include/rmem.h (rmem_polygon_fill_labels) in numpy and plain Python: the
even-odd rule sampled at pixel centres in exact integer arithmetic on 1/256-pixel fixed point, written from the contract and never
from the kernels.  The package does not import it.  Also the quantiser, the painter of a stack (listing order, the later shape
wins), a float crossing-number test that shares nothing with the restatement but the rule, and the polygons the tests fill."""
import numpy as np


def fill(rings_fx, H, W):                       # rings_fx: int arrays [k, 2] in 1/256 px
    tog = np.zeros((H, W + 1), dtype=np.int64)
    for r in rings_fx:
        v = [(int(a), int(b)) for a, b in r]
        for (X0, Y0), (X1, Y1) in zip(v, v[1:] + v[:1]):
            if Y0 == Y1:
                continue
            if Y0 > Y1:
                X0, Y0, X1, Y1 = X1, Y1, X0, Y0
            dY, dX = Y1 - Y0, X1 - X0
            ya, yb = max(0, -((128 - Y0) // 256)), min(H, -((128 - Y1) // 256))
            for y in range(ya, yb):
                num = X0 * dY + (256 * y + 128 - Y0) * dX
                c = min(max(-((128 * dY - num) // (256 * dY)), 0), W)
                tog[y, c] ^= 1
    return (np.cumsum(tog, axis=1)[:, :W] & 1).astype(bool)


def quantise(ring):
    """int64 [k, 2] in 1/256 pixel of a ring given as [k, 2] or flat: numpy.rint on float64, ties to even"""
    return np.rint(256.0 * np.asarray(ring, dtype=np.float64).reshape(-1, 2)).astype(np.int64)


def fill_rings(rings, H, W):
    """bool [H, W] of a shape given as float rings"""
    return fill([quantise(r) for r in rings], H, W)


def paint_stack(frames, H, W):
    """uint8 [n, H, W]: frames[f] = [(value, [ring, ...]), ...], label[shape] = value in listing order, 0 under no shape"""
    out = np.zeros((len(frames), H, W), dtype=np.uint8)
    for f, shapes in enumerate(frames):
        for value, rings in shapes:
            out[f][fill_rings(rings, H, W)] = value
    return out


def crossing_number(rings, H, W):
    """bool [H, W] by the crossing-number test in float64 on the quantised vertices: a pixel is inside iff an odd number of edges
    with y0 <= cy < y1 have the centre on or right of them, the side taken from the sign of a cross product.  Exact while the
    products stay below 2^53, which the small frames of the tests guarantee."""
    cy, cx = np.mgrid[0:H, 0:W]
    cx, cy = 256.0 * cx + 128.0, 256.0 * cy + 128.0
    inside = np.zeros((H, W), dtype=bool)
    for r in rings:
        q = quantise(r).astype(np.float64)
        for (x0, y0), (x1, y1) in zip(q, np.roll(q, -1, axis=0)):
            if y0 == y1:
                continue
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            assert max(abs(x0), abs(x1), abs(y0), abs(y1), cx.max(), cy.max()) < 2.0 ** 25
            inside ^= (y0 <= cy) & (cy < y1) & ((cx - x0) * (y1 - y0) - (cy - y0) * (x1 - x0) >= 0)
    return inside


# ---------------------------------------------------------------------------------------------------------------- polygons
def random_polygon(rng, H, W, k=None, margin=3.0):
    """a ring of k fractional vertices, anywhere from `margin` pixels outside the frame to inside it: usually self-intersecting"""
    k = int(rng.integers(3, 9)) if k is None else k
    return np.stack([rng.uniform(-margin, W + margin, k), rng.uniform(-margin, H + margin, k)], axis=1)


def star(rng, H, W, points=5):
    """a pentagram-like ring round a random centre: every second point of a circle, so the ring crosses itself"""
    cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1.0, max(H, W))
    a = rng.uniform(0, 2 * np.pi) + 2 * np.pi * ((2 * np.arange(points)) % points) / points
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def tie_cases():
    """(name, [ring, ...]) whose vertices and edges hit the sample points exactly; they fit a frame of 7 x 9 and more"""
    sq = [(1.5, 1.5), (4.5, 1.5), (4.5, 4.5), (1.5, 4.5)]
    return [
        ('vertices on pixel centres', [sq]),
        ('vertices on pixel corners', [[(1, 1), (4, 1), (4, 3), (1, 3)]]),
        ('a diagonal through centres', [[(0.5, 0.5), (5.5, 5.5), (0.5, 5.5)]]),
        ('the other diagonal through centres', [[(5.5, 0.5), (5.5, 5.5), (0.5, 5.5)]]),
        ('horizontal edges on sample rows', [[(1.25, 1.5), (6.75, 1.5), (6.75, 3.5), (1.25, 3.5)]]),
        ('vertical edges on centre columns', [[(2.5, 0.25), (5.5, 0.25), (5.5, 6.0), (2.5, 6.0)]]),
        ('repeated vertices', [[p for p in sq for _ in range(2)]]),
        ('a vertex on a sample row between two edges', [[(1, 0), (3, 2.5), (1, 5), (6, 2.5)]]),
        ('zero area, collinear', [[(1, 1), (4, 4), (2.5, 2.5)]]),
        ('zero area, out and back', [[(1.5, 0.5), (1.5, 4.5), (1.5, 0.5)]]),
        ('a ring listed twice cancels', [sq, sq]),
        ('a bow tie', [[(1, 1), (5, 5), (5, 1), (1, 5)]]),
        ('half-way vertices (ties of the quantiser)', [[(1 + 1 / 512, 1 + 1 / 512), (4 + 3 / 512, 1 + 1 / 512), (4 + 3 / 512, 4 + 3 / 512)]]),
        ('an exterior and a hole, one orientation', [[(0, 0), (7, 0), (7, 6), (0, 6)], [(2, 2), (5, 2), (5, 4), (2, 4)]]),
        ('an exterior and a hole, the other', [[(0, 0), (7, 0), (7, 6), (0, 6)], [(2, 2), (2, 4), (5, 4), (5, 2)]]),
    ]


def triangle_fan(rng, H, W, centre='fraction', k=None):
    """(outline ring, [triangle ring, ...]): k >= 5 points of an ellipse at increasing angles (a convex outline that may leave the
    frame) and the triangles (centre, p_i, p_i+1).  centre: 'centre' (a pixel centre), 'corner' (a pixel corner) or 'fraction'.
    The triangles share their quantised vertices, so they partition the outline's fill: every pixel is covered exactly once."""
    k = int(rng.integers(5, 10)) if k is None else k
    cx, cy = float(rng.integers(0, W)), float(rng.integers(0, H))
    if centre == 'centre':
        cx, cy = cx + 0.5, cy + 0.5
    elif centre == 'fraction':
        cx, cy = cx + float(rng.uniform(0, 1)), cy + float(rng.uniform(0, 1))
    a = 2 * np.pi * (np.arange(k) + rng.uniform(0, 0.9, k)) / k       # gaps below 0.76 pi: the centre is inside
    rx, ry = rng.uniform(1.0, W), rng.uniform(1.0, H)
    pts = np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], axis=1)
    return pts, [np.array([(cx, cy), tuple(pts[i]), tuple(pts[(i + 1) % k])]) for i in range(k)]
