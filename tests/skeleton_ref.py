"""numpy restatement of the thinning of label stacks (Guo and Hall 1989, algorithm A1), of the pixel list, of the longest path
through a skeleton component and of evaluator.next_scribbles, written from the rule's text and not from the C code.

Value 0 is background.  For a pixel p of value L != 0 the neighbour bit x_i is 1 iff that neighbour lies inside the frame and holds
L; x1..x8 = E, NE, N, NW, W, SW, S, SE (y grows downward), x9 = x1.  p is deleted in a sub-iteration iff
  G1  X_H = sum_{i=1..4} [x_{2i-1} = 0 and (x_{2i} = 1 or x_{2i+1} = 1)] = 1,
  G2  2 <= min(n1, n2) <= 3,  n1 = sum_{k=1..4} (x_{2k-1} | x_{2k}),  n2 = sum_{k=1..4} (x_{2k} | x_{2k+1}),
  G3  even sub-iterations: (x2 | x3 | !x8) & x1 = 0;  odd ones: (x6 | x7 | !x4) & x5 = 0.
A sub-iteration is synchronous; an iteration is an even sub-iteration and an odd one; the skeleton is the state after the first
iteration in which neither deletes anything."""
from collections import deque

import numpy as np

import edt_ref

# (dy, dx) of x1..x8
NEIGHBOURS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


def tables():
    """bool [2, 256]: tables()[parity][mask], mask bit k = x_{k+1}"""
    t = np.zeros((2, 256), dtype=bool)
    for m in range(256):
        x = [0] + [(m >> k) & 1 for k in range(8)]
        x.append(x[1])
        xh = sum(1 for i in range(1, 5) if x[2 * i - 1] == 0 and (x[2 * i] == 1 or x[2 * i + 1] == 1))
        n1 = sum(x[2 * k - 1] | x[2 * k] for k in range(1, 5))
        n2 = sum(x[2 * k] | x[2 * k + 1] for k in range(1, 5))
        if xh != 1 or not 2 <= min(n1, n2) <= 3:
            continue
        t[0, m] = ((x[2] | x[3] | (1 - x[8])) & x[1]) == 0
        t[1, m] = ((x[6] | x[7] | (1 - x[4])) & x[5]) == 0
    return t


_TABLES = tables()


def masks(a):
    """the neighbour mask of every pixel of a [..., H, W] (0 on background)"""
    a = np.asarray(a, dtype=np.uint8)
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (H + 2, W + 2), dtype=np.uint8)
    p[..., 1:-1, 1:-1] = a
    m = np.zeros(a.shape, dtype=np.int64)
    for k, (dy, dx) in enumerate(NEIGHBOURS):
        nb = p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        m |= ((nb == a) & (a != 0)).astype(np.int64) << k
    return m


def sub_iteration(a, s):
    """(the stack after sub-iteration s, the pixels every frame lost [n]) for a [n, H, W]; [H, W] is one frame"""
    a = np.asarray(a, dtype=np.uint8)
    gone = _TABLES[s & 1][masks(a)] & (a != 0)
    out = np.where(gone, 0, a).astype(np.uint8)
    return out, gone.reshape(-1, *a.shape[-2:]).sum(axis=(1, 2)).astype(np.int64)


def run(a, first, count):
    """(the stack after sub-iterations first .. first + count - 1, lost int64 [n, 2]): lost[f] = (the pixels lost in all of them, in
    the last two -- in the only one if count = 1)"""
    a = np.asarray(a, dtype=np.uint8)
    n = a.reshape(-1, *a.shape[-2:]).shape[0]
    lost = np.zeros((n, 2), dtype=np.int64)
    for s in range(first, first + count):
        a, gone = sub_iteration(a, s)
        lost[:, 0] += gone
        if s >= first + count - 2:
            lost[:, 1] += gone
    return a, lost


def thin(a, max_iterations=None, with_iterations=False):
    """the skeleton; max_iterations = k stops after k iterations.  with_iterations: (skeleton, iterations run, the last one -- the
    one that deleted nothing -- included)"""
    a = np.asarray(a, dtype=np.uint8)
    it = 0
    while max_iterations is None or it < max_iterations:
        a, lost = run(a, 0, 2)
        it += 1
        if not lost[:, 0].any():
            break
    return (a, it) if with_iterations else a


def thin_tiled(a, th, tw, k, count, first=0):
    """`count` sub-iterations of one frame [H, W] evaluated on tiles of th x tw with a halo of k (zeros outside the frame), k
    sub-iterations per round, only the core kept"""
    a = np.asarray(a, dtype=np.uint8)
    H, W = a.shape
    s = first
    while s < first + count:
        m = min(k, first + count - s)
        p = np.zeros((H + 2 * k, W + 2 * k), dtype=np.uint8)
        p[k:k + H, k:k + W] = a
        out = np.empty_like(a)
        for y in range(0, H, th):
            for x in range(0, W, tw):
                region = run(p[y:y + th + 2 * k, x:x + tw + 2 * k], s, m)[0]
                core = region[k:k + th, k:k + tw]
                out[y:y + th, x:x + tw] = core[:min(th, H - y), :min(tw, W - x)]
        a, s = out, s + m
    return a


def pixels(stack, samples=None):
    """(entries int32 [K, 4] = (frame, y, x, value) of the non-zero pixels in raster order frame by frame, totals int32 [n]) and,
    with samples, sampled int32 [K]"""
    s = np.asarray(stack, dtype=np.uint8)
    s = s[None] if s.ndim == 2 else s
    f, y, x = np.nonzero(s)
    entries = np.stack([f, y, x, s[f, y, x]], axis=1).astype(np.int32).reshape(-1, 4)
    totals = (s != 0).sum(axis=(1, 2)).astype(np.int32)
    if samples is None:
        return entries, totals
    return entries, totals, np.asarray(samples).reshape(s.shape)[f, y, x].astype(np.int32)


def _bfs(yx, start):
    index = {(int(y), int(x)): i for i, (y, x) in enumerate(yx)}
    dist = np.full(len(yx), -1, dtype=np.int64)
    parent = np.full(len(yx), -1, dtype=np.int64)
    dist[start] = 0
    q = deque([start])
    while q:
        i = q.popleft()
        y, x = int(yx[i][0]), int(yx[i][1])
        for dy, dx in NEIGHBOURS:
            j = index.get((y + dy, x + dx))
            if j is not None and dist[j] < 0:
                dist[j], parent[j] = dist[i] + 1, i
                q.append(j)
    return dist, parent


def longest_path(yx):
    """yx: the pixels of one 8-connected skeleton component in raster order.  a = the farthest pixel (hops, FIFO breadth-first
    search, neighbours in the order E, NE, N, NW, W, SW, S, SE, the smallest raster index among equals) from the first pixel, b =
    the farthest from a; the parent chain from a to b as int32 [k, 2]"""
    yx = np.asarray(yx, dtype=np.int64).reshape(-1, 2)
    a = int(np.argmax(_bfs(yx, 0)[0]))
    dist, parent = _bfs(yx, a)
    i = int(np.argmax(dist))
    chain = [i]
    while parent[i] >= 0:
        i = int(parent[i])
        chain.append(i)
    return yx[chain[::-1]].astype(np.int32)


def component(yx, start):
    """the rows of yx (raster order) 8-connected to row `start`, in raster order"""
    return np.nonzero(_bfs(np.asarray(yx, dtype=np.int64).reshape(-1, 2), start)[0] >= 0)[0]


def components_count(mask):
    """the number of 8-connected components of a bool frame"""
    yx = np.argwhere(mask)
    seen = np.zeros(len(yx), dtype=bool)
    c = 0
    for i in range(len(yx)):
        if not seen[i]:
            seen[component(yx, i)] = True
            c += 1
    return c


def next_scribbles(pred, gt, num_objs, min_depth2=4):
    """per frame {object id: {'positive', 'path', 'depth2'}}: evaluator.next_scribbles restated"""
    pred, gt = np.asarray(pred, dtype=np.uint8), np.asarray(gt, dtype=np.uint8)
    if pred.ndim == 2:
        pred, gt = pred[None], gt[None]
    lists = []
    for stack in (np.where(pred != gt, gt, 0), np.where(pred != gt, pred, 0)):       # false negatives, false positives
        stack = np.where(stack > num_objs, 0, stack).astype(np.uint8)
        d2 = edt_ref.edt(stack, None, True)
        e, _, s = pixels(thin(stack), d2)
        lists.append((e, s))
    out = []
    for f in range(pred.shape[0]):
        frame = {}
        for v in range(1, num_objs + 1):
            best = None
            for positive, (e, s) in ((True, lists[0]), (False, lists[1])):
                rows = np.nonzero((e[:, 0] == f) & (e[:, 3] == v))[0]
                if rows.size == 0:
                    continue
                k = int(np.argmax(s[rows]))                          # the first in raster order among equals
                depth = int(s[rows[k]])
                if best is None or depth >= best[0]:                  # the false positive on equal depth
                    best = (depth, positive, e[rows][:, 1:3], k)
            if best is None or best[0] < min_depth2:
                continue
            depth, positive, yx, k = best
            frame[v] = {'positive': positive, 'path': longest_path(yx[component(yx, k)]), 'depth2': depth}
        out.append(frame)
    return out


def blobs(seed, n, H, W, values=3, count=6):
    """a stack of overlapping discs and boxes of values 1..values on background"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.zeros((n, H, W), dtype=np.uint8)
    for f in range(n):
        for _ in range(count):
            cy, cx, r, v = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W) // 3 + 2)), rng.integers(1, values + 1)
            if rng.integers(0, 2):
                a[f][(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = v
            else:
                a[f][(abs(y - cy) <= r) & (abs(x - cx) <= 2 * r)] = v
    return a
