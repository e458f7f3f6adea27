"""Sequential restatement of the polygon contract of include/rmem.h (rmem_label_polygons) in numpy and plain Python: edges, the
successor rule, rings, vertices and area2, written from the contract's tables and never from the kernels.  The package does not
import it.  Also the rasteriser the round-trip checks use, and the contents the tests and the measurement script trace."""
import numpy as np

# side -> (from corner, to corner) as offsets (dx, dy) from the pixel's top-left corner (x, y)
CORNERS = {0: ((0, 0), (1, 0)), 1: ((1, 0), (1, 1)), 2: ((1, 1), (0, 1)), 3: ((0, 1), (0, 0))}
# side -> the neighbour across it, and the pixels A (ahead on the right) and B (ahead on the left) as (dy, dx)
ACROSS = {0: (-1, 0), 1: (0, 1), 2: (1, 0), 3: (0, -1)}
AHEAD = {0: ((0, 1), (-1, 1)), 1: ((1, 0), (1, 1)), 2: ((0, -1), (1, -1)), 3: ((-1, 0), (-1, -1))}
ST_CAPACITY = 1


def _objects(frame, num_objs):
    frame = np.asarray(frame).astype(np.int64)
    assert frame.ndim == 2
    return np.where(frame > num_objs, 0, frame)


def edges(frame, num_objs):
    """the sorted edge ids of a frame"""
    obj = _objects(frame, num_objs)
    H, W = obj.shape
    pad = np.zeros((H + 2, W + 2), dtype=np.int64)                  # outside the frame nothing holds an object's value
    pad[1:-1, 1:-1] = obj
    out = []
    for s, (dy, dx) in ACROSS.items():
        owns = (obj != 0) & (pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] != obj)
        out.append(np.flatnonzero(owns) * 4 + s)
    return sorted(int(e) for e in np.concatenate(out))


def _padded(obj):
    """rows of the frame with a border of 0 around it, as lists: outside the frame nothing holds an object's value"""
    H, W = obj.shape
    pad = np.zeros((H + 2, W + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = obj
    return pad.tolist()


def successor(pad, W, e, connectivity):
    """pad: _padded(frame); pixel (y, x) is pad[y + 1][x + 1]"""
    s, p = e & 3, e >> 2
    y, x = divmod(p, W)
    v = pad[y + 1][x + 1]
    (ay, ax), (by, bx) = AHEAD[s]
    a, b = pad[y + 1 + ay][x + 1 + ax] == v, pad[y + 1 + by][x + 1 + bx] == v
    if connectivity == 8:
        move = 'left' if b else ('straight' if a else 'right')
    else:
        move = 'right' if not a else ('straight' if not b else 'left')
    if move == 'right':
        return p * 4 + (s + 1) % 4
    if move == 'straight':
        return ((y + ay) * W + x + ax) * 4 + s
    return ((y + by) * W + x + bx) * 4 + (s + 3) % 4


def trace(frame, num_objs, connectivity):
    """the rings of one frame in the order of their start edges: dicts with 'value', 'start', 'edges' (the count), 'area2' and
    'verts' (int32 [k, 2], (x, y))"""
    assert connectivity in (4, 8)
    obj = _objects(frame, num_objs)
    W = obj.shape[1]
    todo = edges(frame, num_objs)
    pad = _padded(obj)
    seen = set()
    rings = []
    for start in todo:                                              # ascending: the first edge met of a ring is its smallest
        if start in seen:
            continue
        walk, e = [], start
        while e not in seen:
            seen.add(e)
            walk.append(e)
            e = successor(pad, W, e, connectivity)
        assert e == start, 'the successor rule is no permutation here'
        verts = []
        for k, e in enumerate(walk):
            if (e & 3) != (walk[k - 1] & 3):                        # k = 0: the predecessor of the start is the ring's last edge
                y, x = divmod(e >> 2, W)
                dx, dy = CORNERS[e & 3][0]
                verts.append((x + dx, y + dy))
        area2 = sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(verts, verts[1:] + verts[:1]))
        y, x = divmod(start >> 2, W)
        rings.append({'value': int(obj[y, x]), 'start': start, 'edges': len(walk), 'area2': int(area2),
                      'verts': np.array(verts, dtype=np.int32).reshape(-1, 2)})
    return rings


def arrays(stack, num_objs, connectivity):
    """(rings int32 [R, 8], verts int32 [V, 2], counts int32 [4]) of a stack as rmem_label_polygons writes them when they fit"""
    rows, verts, E, V = [], [], 0, 0
    for f, frame in enumerate(np.asarray(stack)):
        for r in trace(frame, num_objs, connectivity):
            rows.append((f, r['value'], V, len(r['verts']), r['area2'], r['start'], r['edges'], 0))
            verts.append(r['verts'])
            E += r['edges']
            V += len(r['verts'])
    rings = np.array(rows, dtype=np.int32).reshape(-1, 8)
    verts = np.concatenate(verts).astype(np.int32) if verts else np.zeros((0, 2), dtype=np.int32)
    return rings, verts, np.array([E, len(rows), len(verts), 0], dtype=np.int32)


def rasterise(rings, value, H, W):
    """bool [H, W]: the pixels inside the rings of `value` (trace()'s dicts, or any dicts with 'value' and 'verts').  Every
    vertical ring edge at column x toggles the pixels of its rows at columns >= x: XOR the toggles, then the parity of the
    cumulative sum along x."""
    toggles = np.zeros((H, W + 1), dtype=np.int64)
    for r in rings:
        if r['value'] != value:
            continue
        v = [tuple(int(c) for c in p) for p in r['verts']]
        for (x0, y0), (x1, y1) in zip(v, v[1:] + v[:1]):
            if x0 == x1:
                toggles[min(y0, y1):max(y0, y1), x0] ^= 1
    return (np.cumsum(toggles, axis=1)[:, :W] & 1).astype(bool)


def rings_of(rings, verts, frame):
    """trace()'s dicts of one frame from the arrays of a device call (or of arrays())"""
    return [{'value': int(r[1]), 'start': int(r[5]), 'edges': int(r[6]), 'area2': int(r[4]), 'verts': verts[r[2]:r[2] + r[3]]}
            for r in rings if r[0] == frame]


# ---------------------------------------------------------------------------------------------------------------- contents
def speckle(stack, seed, fraction, num_objs):
    """`fraction` of the pixels set to a random value in 0..num_objs"""
    rng = np.random.default_rng(seed)
    out = np.array(stack, copy=True)
    hit = rng.random(out.shape) < fraction
    out[hit] = rng.integers(0, num_objs + 1, size=int(hit.sum()), dtype=np.uint8)
    return out


def noise(seed, n, H, W, values=4):
    return np.random.default_rng(seed).integers(0, values, size=(n, H, W), dtype=np.uint8)


def checkerboard(n, H, W):
    y, x = np.mgrid[0:H, 0:W]
    a = np.where((y + x) & 1, 1, 2).astype(np.uint8)
    return np.stack([a if f % 2 == 0 else 3 - a for f in range(n)])


def stripes(n, H, W):
    """one-pixel stripes, across in even frames and down in odd ones"""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([((y if f % 2 == 0 else x) & 1).astype(np.uint8) * (1 + f % 3) for f in range(n)])


def serpentine(n, H, W):
    """one object that fills every second row and joins the rows at alternating ends: a single ring with nearly every edge"""
    a = np.zeros((H, W), dtype=np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        a[y, W - 1 if k % 2 == 0 else 0] = 1
    return np.stack([a] * n)


def concentric(n, H, W):
    """rectangular rings one pixel wide, two pixels apart, of alternating objects 1 and 2: holes inside holes"""
    y, x = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    a = np.where(d % 2 == 0, 1 + (d // 2) % 2, 0).astype(np.uint8)
    return np.stack([a] * n)


def nest(n, H, W):
    """object 1 with a hole that holds object 2 with a hole that holds object 3, away from the frame's edge where there is room"""
    a = np.zeros((H, W), dtype=np.uint8)
    for k, v in enumerate((1, 0, 2, 0, 3)):
        m = k + (1 if min(H, W) > 10 else 0)
        if H - 2 * m > 0 and W - 2 * m > 0:
            a[m:H - m, m:W - m] = v
    return np.stack([a] * n)


def with_other_values(stack, num_objs, seed):
    """values above num_objs (not objects) written over a tenth of the pixels"""
    rng = np.random.default_rng(seed)
    out = np.array(stack, copy=True)
    hit = rng.random(out.shape) < 0.1
    out[hit] = rng.integers(num_objs + 1, 256, size=int(hit.sum()), dtype=np.uint8)
    return out
