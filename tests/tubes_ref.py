"""The contract of the label tubes (include/rmem.h, rmem_label_tubes ... rmem_label_tube_clean) restated independently of the
kernels, twice: with scipy.ndimage.label on the 3-D structures (tubes), and with a plain Python union-find over the pieces of
components_ref.roots (tubes_by_pieces).  Lineage, events, index, table and the clean rule in numpy, and the contents the tests
share.  Tests only: the package never imports scipy."""
import numpy as np
from scipy import ndimage

import census_ref
import components_ref as C


def structure(connectivity, temporal):
    """the 3 x 3 x 3 structure: the centre plane is the pieces' connectivity, the outer planes the centre voxel or the full 3 x 3"""
    assert connectivity in (4, 8) and temporal in (1, 9)
    s = np.zeros((3, 3, 3), dtype=bool)
    s[1] = C.S8 if connectivity == 8 else C.S4
    if temporal == 9:
        s[0] = s[2] = True
    else:
        s[0, 1, 1] = s[2, 1, 1] = True
    return s


def tubes(labels, connectivity=8, temporal=1):
    """int32 [n, H, W]: the global index of the first voxel of every voxel's tube, by scipy.ndimage.label value by value"""
    labels = np.asarray(labels)
    index = np.arange(labels.size, dtype=np.int64).reshape(labels.shape)
    out = np.empty(labels.shape, dtype=np.int32)
    for v in np.unique(labels):
        lab, k = ndimage.label(labels == v, structure=structure(connectivity, temporal))
        first = ndimage.minimum(index, lab, index=np.arange(1, k + 1))
        m = lab > 0
        out[m] = np.asarray(first, dtype=np.int64)[lab[m] - 1]
    return out


def pairs(labels, r, f, temporal):
    """int64 [k, 2]: the distinct (root on frame f, root on frame f - 1) of linked pieces"""
    H, W = labels.shape[1:]
    reach = 1 if temporal == 9 else 0
    found = [np.empty(0, dtype=np.int64)]
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yp, xp = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            m = labels[f][ys, xs] == labels[f - 1][yp, xp]
            found.append(np.unique(r[f][ys, xs][m].astype(np.int64) * (H * W) + r[f - 1][yp, xp][m]))
    both = np.unique(np.concatenate(found))
    return np.stack([both // (H * W), both % (H * W)], axis=1)


def tubes_by_pieces(labels, connectivity=8, temporal=1, r=None):
    """the same by a union-find in plain Python over the pieces (frame, root) and their links"""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    HW = H * W
    r = C.roots(labels, connectivity) if r is None else r
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for f in range(1, n):
        for a, b in pairs(labels, r, f, temporal).tolist():
            x, y = find(f * HW + a), find((f - 1) * HW + b)
            if x != y:
                parent[max(x, y)] = min(x, y)                       # the smaller index wins: a set's representative is its first voxel
    piece = r.astype(np.int64) + (np.arange(n, dtype=np.int64) * HW)[:, None, None]
    ids = np.unique(piece)
    first = np.array([find(int(g)) for g in ids], dtype=np.int64)
    return first[np.searchsorted(ids, piece)].astype(np.int32)


def lineage(labels, r, temporal=1):
    """int32 [n, H * W, 4]: (prev_min, prev_max, next_min, next_max) at roots, (H * W, -1, H * W, -1) elsewhere"""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    HW = H * W
    links = np.empty((n, HW, 4), dtype=np.int32)
    links[:] = (HW, -1, HW, -1)
    for f in range(1, n):
        p = pairs(labels, r, f, temporal)
        a, b = p[:, 0], p[:, 1]
        np.minimum.at(links[f, :, 0], a, b)
        np.maximum.at(links[f, :, 1], a, b)
        np.minimum.at(links[f - 1, :, 2], b, a)
        np.maximum.at(links[f - 1, :, 3], b, a)
    return links


def events(labels, r, links):
    """int32 [n, 256, 4]: (born, ended, splitting, merging) pieces per frame and value"""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    out = np.zeros((n, 256, 4), dtype=np.int32)
    flat = np.arange(H * W)
    for f in range(n):
        is_root = r[f].reshape(-1) == flat
        v = labels[f].reshape(-1)[is_root].astype(np.int64)
        k = links[f][is_root]
        flags = (np.full(len(v), f >= 1) & (k[:, 1] < 0), np.full(len(v), f <= n - 2) & (k[:, 3] < 0),
                 (k[:, 3] >= 0) & (k[:, 2] != k[:, 3]), (k[:, 1] >= 0) & (k[:, 0] != k[:, 1]))
        for c, m in enumerate(flags):
            out[f, :, c] = np.bincount(v[m], minlength=256)
    return out


def index(t):
    """(rank int32 [n, H, W], total): the position of every tube id among all ids at its first voxel, -1 elsewhere"""
    flat = t.reshape(-1)
    first = flat == np.arange(flat.size)
    rank = np.full(flat.size, -1, dtype=np.int32)
    rank[first] = np.arange(int(first.sum()), dtype=np.int32)
    return rank.reshape(t.shape), int(first.sum())


def table(labels, r, S, t):
    """int32 [T, 10]: (first, value, voxels, pieces, f_first, f_last, nb_min, nb_max, border, peak_area) per tube in ascending id"""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    HW = H * W
    ids = np.unique(t).astype(np.int64)
    out = np.zeros((len(ids), 10), dtype=np.int32)
    out[:, 0] = ids
    out[:, 1] = labels.reshape(-1)[ids]
    out[:, 4] = n
    out[:, 5] = -1
    out[:, 6] = 256
    out[:, 7] = -1
    for f in range(n):
        roots_f = np.nonzero(r[f].reshape(-1) == np.arange(HW))[0]
        row = np.searchsorted(ids, t[f].reshape(-1)[roots_f])
        area, lo, hi, border = (S[f][roots_f, k] for k in range(4))
        np.add.at(out[:, 2], row, area)
        np.add.at(out[:, 3], row, 1)
        np.minimum.at(out[:, 4], row, f)
        np.maximum.at(out[:, 5], row, f)
        np.minimum.at(out[:, 6], row, lo)
        np.maximum.at(out[:, 7], row, hi)
        np.maximum.at(out[:, 8], row, border)
        np.maximum.at(out[:, 9], row, area)
    return out


def clean(labels, min_frames=0, max_hole_frames=0, connectivity=8, temporal=1, r=None, S=None, t=None, T=None):
    """the rule, voxel set by voxel set, from the input's pieces and tubes"""
    labels = np.asarray(labels)
    n = labels.shape[0]
    r = C.roots(labels, connectivity) if r is None else r
    S = C.stats(labels, connectivity, r)[0] if S is None else S
    t = tubes(labels, connectivity, temporal) if t is None else t
    T = table(labels, r, S, t) if T is None else T
    row = T[np.searchsorted(T[:, 0], t)]                            # [n, H, W, 10]
    f_first, f_last = row[..., 4], row[..., 5]
    life = f_last - f_first + 1
    closed = (f_first >= 1) & (f_last <= n - 2)
    out = labels.copy()
    for f in range(n):
        piece = S[f][r[f].astype(np.int64)]                         # [H, W, 4]
        one = piece[..., 1] == piece[..., 2]
        flicker = (labels[f] != 0) & closed[f] & (life[f] < min_frames)
        hole = (labels[f] == 0) & closed[f] & (life[f] <= max_hole_frames) & (row[f][..., 8] == 0) & (row[f][..., 6] == row[f][..., 7])
        out[f][flicker & one] = piece[..., 1][flicker & one]
        out[f][flicker & ~one] = 0
        out[f][hole] = row[f][..., 6][hole]
    return out


def everything(labels, connectivity, temporal):
    """dict of every reference output of one stack, read only"""
    labels = np.asarray(labels)
    r = C.roots(labels, connectivity)
    S, _ = C.stats(labels, connectivity, r)
    t = tubes(labels, connectivity, temporal)
    links = lineage(labels, r, temporal)
    rank, total = index(t)
    out = dict(roots=r, stats=S, tubes=t, links=links, events=events(labels, r, links), rank=rank, total=total, table=table(labels, r, S, t))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- contents
BAR = ((1, 1, 1, 1, 1, 1), (1, 1, 0, 0, 1, 1), (1, 1, 0, 0, 1, 1), (1, 1, 1, 1, 1, 1))     # the split / merge bar, frame by frame
CONTENTS = ('drift', 'noise', 'one', 'checker', 'flip', 'bars', 'stairs')


def content(name, n, H, W):
    """uint8 [n, H, W], seeded by the shape alone"""
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    f, y, x = np.mgrid[0:n, 0:H, 0:W]
    if name == 'drift':                                             # blobs drifting by (1, 2) pixels per frame, and 2-frame specks
        a = census_ref.blobs(H * W + n, n, H, W)
        for k in range(12):
            f0 = k % max(n - 1, 1)                                  # every first frame in turn: open at either end, and closed
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            a[f0:f0 + 2, y0:y0 + 2, x0:x0 + 2] = int(rng.integers(1, 11))
    elif name == 'noise':                                           # three values: nearly every voxel ends a piece
        a = rng.integers(0, 3, (n, H, W)).astype(np.uint8)
    elif name == 'one':
        a = np.full((n, H, W), 7, dtype=np.uint8)
    elif name == 'checker':                                         # the same checkerboard on every frame
        a = ((y + x) % 2).astype(np.uint8)
    elif name == 'flip':                                            # inverted on alternate frames: under (4, 1) nothing links
        a = ((y + x + f) % 2).astype(np.uint8)
    elif name == 'bars':                                            # the bar in cells of 2 x 8 pixels, whole / split / split / whole
        a = np.zeros((n, H, W), dtype=np.uint8)
        bar = np.array(BAR, dtype=np.uint8)
        for k in range(n):
            row = np.zeros(8, dtype=np.uint8)
            row[1:7] = bar[k % 4]
            a[k, 0::2, :] = np.tile(row, W // 8 + 1)[:W]
    else:                                                           # 'stairs': frame k holds a run on row k * sy and the step down to
        a = np.zeros((n, H, W), dtype=np.uint8)                     # the next run; consecutive frames share one pixel only
        sy, sx = max((H - 1) // max(n, 1), 1), max((W - 1) // max(n, 1), 1)
        for k in range(n):
            y0, y1 = min(k * sy, H - 1), min((k + 1) * sy, H - 1)
            x0, x1 = min(k * sx, W - 1), min((k + 1) * sx, W - 1)
            a[k, y0, x0:x1 + 1] = 1
            a[k, y0:y1 + 1, x1] = 1
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a
