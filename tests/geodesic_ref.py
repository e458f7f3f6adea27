"""Host restatement of the geodesic nearest-site transform (include/rmem.h: rmem_label_geodesic_*), twice and independently:
a vectorised 8-neighbour Jacobi iteration on packed int64 keys (cost << 26) | index, and a heapq Dijkstra on (cost, index) pairs.
Both return the packed keys of a stack; finish() turns keys into the three outputs.  And the generators of the frames, label
stacks and site sets the tests use.

The graph: the 8-connected grid of a frame, the edge between neighbours p and q costs spatial * s + colour * sum_c |I_c(p) -
I_c(q)|, s = 5 for an axial step and 7 for a diagonal one.  key(p) = the lexicographic minimum over the sites s of (cheapest cost
s -> p, flat index of s)."""
import heapq

import numpy as np

SENTINEL = 2 ** 31 - 1
MAX_COST = 2 ** 30
SHIFT = 26
MASK = (1 << SHIFT) - 1
NOKEY = (SENTINEL << SHIFT) | MASK
STEPS = ((0, 1, 5), (0, -1, 5), (1, 0, 5), (-1, 0, 5), (1, 1, 7), (1, -1, 7), (-1, 1, 7), (-1, -1, 7))


def bits(values):
    w = [0] * 8
    for v in values:
        w[v >> 5] |= 1 << (v & 31)
    return w


def channels(labels, image):
    """the image as int64 [n, H, W, C] next to labels as [n, H, W]"""
    a = labels[None] if labels.ndim == 2 else labels
    im = np.asarray(image, dtype=np.int64)
    if im.shape == labels.shape:
        im = im[..., None]
    return a, im.reshape(a.shape + (im.shape[-1],))


def initial(a, sites):
    n, H, W = a.shape
    idx = np.broadcast_to(np.arange(H * W, dtype=np.int64).reshape(H, W), a.shape)
    return np.where(np.isin(a, list(sites)), idx, NOKEY)


def jacobi(labels, image, sites, spatial=1, colour=1, limit=-1):
    """packed int64 keys [n, H, W]: every pixel takes the minimum of its key and its eight neighbours' keys plus the edge, all at
    once, until nothing changes; a candidate above `limit` (>= 0) is dropped where it arises"""
    a, im = channels(labels, image)
    n, H, W = a.shape
    K = np.full((n, H + 2, W + 2), NOKEY, dtype=np.int64)
    K[:, 1:-1, 1:-1] = initial(a, sites)
    P = np.zeros((n, H + 2, W + 2, im.shape[-1]), dtype=np.int64)
    P[:, 1:-1, 1:-1] = im
    core = P[:, 1:-1, 1:-1]
    shifted = []
    for dy, dx, s in STEPS:
        w = spatial * s + colour * np.abs(core - P[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]).sum(axis=-1)
        shifted.append((dy, dx, w << SHIFT))
    while True:
        new = K[:, 1:-1, 1:-1].copy()
        for dy, dx, w in shifted:
            nb = K[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
            cand = np.where((nb >> SHIFT) == SENTINEL, NOKEY, nb + w)
            if limit >= 0:
                cand = np.where((cand >> SHIFT) > limit, NOKEY, cand)
            np.minimum(new, cand, out=new)
        if np.array_equal(new, K[:, 1:-1, 1:-1]):
            return new.reshape(labels.shape)
        K[:, 1:-1, 1:-1] = new


def dijkstra(labels, image, sites, spatial=1, colour=1, limit=-1):
    """the same keys from a heap of (cost, index of the site, pixel): independent of jacobi down to the weights"""
    a, im = channels(labels, image)
    n, H, W = a.shape
    out = np.empty(a.shape, dtype=np.int64)
    for f in range(n):
        lab, I = a[f].reshape(-1).tolist(), im[f].reshape(H * W, -1).tolist()
        best = [None] * (H * W)
        heap = [(0, p, p) for p in range(H * W) if lab[p] in sites]
        for _, s, p in heap:
            best[p] = (0, s)
        heapq.heapify(heap)
        while heap:
            c, s, p = heapq.heappop(heap)
            if best[p] != (c, s):
                continue
            y, x = divmod(p, W)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if (dy or dx) and 0 <= yy < H and 0 <= xx < W:
                        q = yy * W + xx
                        cand = (c + spatial * (7 if dy and dx else 5) + colour * sum(abs(u - v) for u, v in zip(I[p], I[q])), s)
                        if (limit < 0 or cand[0] <= limit) and (best[q] is None or cand < best[q]):
                            best[q] = cand
                            heapq.heappush(heap, cand + (q,))
        out[f] = np.array([NOKEY if b is None else (b[0] << SHIFT) | b[1] for b in best], dtype=np.int64).reshape(H, W)
    return out.reshape(labels.shape)


def finish(labels, keys, fill=None, max_cost=-1):
    """(index int32, cost int32, taken uint8) from the keys: -1 and SENTINEL where no site is within max_cost (cost == max_cost
    counts); taken = the label at index where the pixel's own label is in fill (None: every value) and a site was found"""
    cost, idx = keys >> SHIFT, keys & MASK
    found = (cost != SENTINEL) & ((max_cost < 0) | (cost <= max_cost))
    index = np.where(found, idx, -1).astype(np.int32)
    a = labels[None] if labels.ndim == 2 else labels
    n = a.shape[0]
    at = np.take_along_axis(a.reshape(n, -1), np.where(found, idx, 0).reshape(n, -1), axis=1).reshape(labels.shape)
    fills = found if fill is None else found & np.isin(labels, list(fill))
    return index, np.where(found, cost, SENTINEL).astype(np.int32), np.where(fills, at, labels).astype(np.uint8)


def chamfer(H, W, y0, x0):
    """the 5-7 chamfer distance of every pixel of a frame to (y0, x0), by hand: the diagonal steps first, the rest axial"""
    y, x = np.mgrid[0:H, 0:W]
    dy, dx = np.abs(y - y0), np.abs(x - x0)
    return 7 * np.minimum(dy, dx) + 5 * np.abs(dy - dx)


# ------------------------------------------------------------------------------------------------------------- generators
IMAGES = ('uniform', 'random', 'step-1', 'step', 'step+1', 'wall')
LABELS = ('sparse', 'blobs', 'ends')
SITE_SETS = ((3,), (1, 2, 3), (0,), (255,), ())


def make_image(kind, shape, C, tw, seed=0):
    """uint8 [n, H, W] (C = 1) or [n, H, W, 3]: uniform; random bytes; a vertical step edge whose first bright column is tw - 1, tw
    or tw + 1 (the tile boundary and one pixel either side); a bright one-pixel wall at column W // 2 with a single gap in its
    last-but-one row (the far tile for a site near the top)"""
    n, H, W = shape
    rng = np.random.default_rng(seed + n * 7919 + H * 131 + W + 17 * C)
    if kind == 'random':
        g = rng.integers(0, 256, (n, H, W, C))
    else:
        v = np.full((n, H, W), 90, dtype=np.int64)
        if kind.startswith('step'):
            v[:] = 40
            v[:, :, tw + {'step-1': -1, 'step': 0, 'step+1': 1}[kind]:] = 200
        elif kind == 'wall':
            v[:] = 0
            v[:, :, W // 2] = 255
            v[:, max(H - 2, 0), W // 2] = 0
        elif kind != 'uniform':
            raise KeyError(kind)
        g = np.stack([v, 255 - v, v // 2][:C], axis=-1)
    g = np.ascontiguousarray(g.astype(np.uint8))
    return g[..., 0] if C == 1 else g


def make_labels(kind, shape, seed=0):
    """uint8 [n, H, W]: sparse single pixels of 1, 2, 3 and 255; blobs (rectangles of 1, 2, 3 and 255); a 3 at index 0 and at
    index H * W - 1 of every frame"""
    n, H, W = shape
    rng = np.random.default_rng(seed + n * 104729 + H * 257 + W)
    a = np.zeros(shape, dtype=np.uint8)
    if kind == 'sparse':
        for v in (1, 2, 3, 255):
            for f in range(n):
                for p in rng.integers(0, H * W, max(1, H * W // 1500)):
                    a[f].reshape(-1)[p] = v
    elif kind == 'blobs':
        for f in range(n):
            for v in (1, 2, 3, 255):
                y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
                a[f, y:y + 1 + H // 6, x:x + 1 + W // 7] = v
    elif kind == 'ends':
        a.reshape(n, -1)[:, [0, -1]] = 3
    else:
        raise KeyError(kind)
    return a


def serpentine(shape):
    """(labels, image): walls of 255 at every column x % 8 == 7, one pixel wide, open alternately in the first and in the last
    row; one site (value 3) at index 0.  With a dear colour term the cheapest path winds through every corridor."""
    n, H, W = shape
    image = np.zeros(shape, dtype=np.uint8)
    for k, x in enumerate(range(7, W, 8)):
        image[:, :, x] = 255
        image[:, H - 1 if k % 2 == 0 else 0, x] = 0
    labels = np.zeros(shape, dtype=np.uint8)
    labels[:, 0, 0] = 3
    return labels, image
