"""The contract of the connected components (include/rmem.h, rmem_label_components / rmem_label_component_stats / rmem_label_clean)
restated with scipy.ndimage.label, frame by frame and value by value, independently of the kernels: roots, stats, table, clean.
Tests only: the package never imports scipy."""
import numpy as np
from scipy import ndimage

S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
S8 = np.ones((3, 3), dtype=bool)


def _structure(connectivity):
    assert connectivity in (4, 8)
    return S8 if connectivity == 8 else S4


def _frame_roots(frame, connectivity):
    """int32 [H, W]: the flat index of the first raster pixel of every pixel's component"""
    H, W = frame.shape
    flat = np.arange(H * W, dtype=np.int64).reshape(H, W)
    out = np.empty((H, W), dtype=np.int32)
    for v in np.unique(frame):
        lab, k = ndimage.label(frame == v, structure=_structure(connectivity))
        first = ndimage.minimum(flat, lab, index=np.arange(1, k + 1))          # per component: its smallest flat index
        m = lab > 0
        out[m] = np.asarray(first, dtype=np.int64)[lab[m] - 1]
    return out


def roots(labels, connectivity=8):
    labels = np.asarray(labels)
    return np.stack([_frame_roots(fr, connectivity) for fr in labels])


def _neighbour_planes(frame, connectivity):
    """for every neighbour offset: (the neighbour's value, or -1 outside the frame) as int32 [H, W]"""
    H, W = frame.shape
    pad = np.full((H + 2, W + 2), -1, dtype=np.int32)
    pad[1:-1, 1:-1] = frame
    st = _structure(connectivity)
    return [pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and st[dy + 1, dx + 1]]


def _frame_stats(frame, r, connectivity):
    H, W = frame.shape
    HW = H * W
    me = frame.astype(np.int32)
    rf = r.reshape(-1).astype(np.int64)
    stats = np.empty((HW, 4), dtype=np.int32)
    stats[:] = (0, 256, -1, 0)
    lo = np.full(HW, 256, dtype=np.int32)
    hi = np.full(HW, -1, dtype=np.int32)
    for nb in _neighbour_planes(frame, connectivity):
        other = ((nb >= 0) & (nb != me)).reshape(-1)
        np.minimum.at(lo, rf[other], nb.reshape(-1)[other])
        np.maximum.at(hi, rf[other], nb.reshape(-1)[other])
    edge = np.zeros((H, W), dtype=bool)
    edge[0] = edge[-1] = True
    edge[:, 0] = edge[:, -1] = True
    area = np.bincount(rf, minlength=HW)
    border = np.bincount(rf, weights=edge.reshape(-1), minlength=HW) > 0
    is_root = area > 0
    stats[is_root, 0] = area[is_root]
    stats[is_root, 1] = lo[is_root]
    stats[is_root, 2] = hi[is_root]
    stats[is_root, 3] = border[is_root]
    table = np.empty((256, 3), dtype=np.int32)
    table[:] = (0, 0, -1)
    vals = frame.reshape(-1)
    for p in np.nonzero(is_root)[0]:                                # ascending roots: the first of the largest stays
        v = int(vals[p])
        table[v, 0] += 1
        if area[p] > table[v, 1]:
            table[v, 1], table[v, 2] = area[p], p
    return stats, table


def stats(labels, connectivity=8, r=None):
    """(stats int32 [n, H * W, 4], table int32 [n, 256, 3])"""
    labels = np.asarray(labels)
    r = roots(labels, connectivity) if r is None else r
    both = [_frame_stats(fr, rr, connectivity) for fr, rr in zip(labels, r)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def clean(labels, max_hole_area=0, max_sprinkle_area=0, keep_largest=False, connectivity=8, r=None, st=None):
    """the rule, pixel set by pixel set, from the input's components"""
    labels = np.asarray(labels)
    r = roots(labels, connectivity) if r is None else r
    S, T = stats(labels, connectivity, r) if st is None else st
    out = labels.copy()
    for f in range(labels.shape[0]):
        fr, rf = labels[f], r[f].astype(np.int64)
        area, lo, hi, border = (S[f][rf, k] for k in range(4))
        one = lo == hi
        hole = (fr == 0) & (area <= max_hole_area) & (border == 0) & one
        gone = (fr != 0) & (area <= max_sprinkle_area)
        if keep_largest:
            gone |= (fr != 0) & (rf != T[f][fr.astype(np.int64), 2])
        out[f][hole] = lo[hole]
        out[f][gone & one] = lo[gone & one]
        out[f][gone & ~one] = 0
    return out
