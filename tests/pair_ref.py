"""numpy restatement of the pair census and of what is read from it: written from include/rmem.h and the definitions, independently
of rmem_ocu_amd.pairs.  pair_iou / track_iou work on boolean masks of the label maps, never through the table; assign tries every
one-to-one assignment."""
import itertools

import numpy as np


def census(a, b, num_a, num_b):
    """int32 [n, num_a + 2, num_b + 2]: pixels of frame f with min(a, num_a + 1) == i and min(b, num_b + 1) == j"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 3
    out = np.empty((a.shape[0], num_a + 2, num_b + 2), dtype=np.int32)
    for f in range(a.shape[0]):
        key = np.minimum(a[f].astype(np.int64), num_a + 1) * (num_b + 2) + np.minimum(b[f].astype(np.int64), num_b + 1)
        out[f] = np.bincount(key.reshape(-1), minlength=(num_a + 2) * (num_b + 2)).reshape(num_a + 2, num_b + 2)
    return out


def inter_union(a, b, num_a, num_b, drop_other_b=True):
    """(inter, union) int64 [n, num_a, num_b] from boolean masks: object i of a against object j of b over the pixels that count
    (all of them, or with drop_other_b those where b <= num_b)"""
    a, b = np.asarray(a), np.asarray(b)
    n = a.shape[0]
    inter = np.zeros((n, num_a, num_b), dtype=np.int64)
    union = np.zeros((n, num_a, num_b), dtype=np.int64)
    for f in range(n):
        counts = (b[f] <= num_b) if drop_other_b else np.ones(b[f].shape, dtype=bool)
        for i in range(1, num_a + 1):
            ma = (a[f] == i) & counts
            for j in range(1, num_b + 1):
                mb = (b[f] == j) & counts
                inter[f, i - 1, j - 1] = np.count_nonzero(ma & mb)
                union[f, i - 1, j - 1] = np.count_nonzero(ma | mb)
    return inter, union


def pair_iou(a, b, num_a, num_b, drop_other_b=True):
    inter, union = inter_union(a, b, num_a, num_b, drop_other_b)
    iou = np.full(inter.shape, np.nan)
    nz = union > 0
    iou[nz] = inter[nz] / union[nz]
    return iou, inter, union


def track_iou(a, b, num_a, num_b, frames=None, drop_other_b=True):
    inter, union = inter_union(a, b, num_a, num_b, drop_other_b)
    if frames is not None:
        inter, union = inter[frames], union[frames]
    i, u = inter.sum(axis=0), union.sum(axis=0)
    out = np.zeros(i.shape)
    nz = u > 0
    out[nz] = i[nz] / u[nz]
    return out


def full_assignments(R, C):
    """every list of min(R, C) pairs (row, column), rows ascending, no row and no column twice"""
    if R <= C:
        for cols in itertools.permutations(range(C), R):
            yield list(zip(range(R), cols))
    else:
        for rows in itertools.permutations(range(R), C):
            yield sorted(zip(rows, range(C)))


def assign(score, minimum=0.0):
    """Brute force: the full assignment of the largest total, the smallest list among equals, pairs not above minimum left out.
    Exact for scores whose sums are exact (the tests use multiples of 1/8)."""
    score = np.asarray(score, dtype=np.float64)
    best, best_total = None, None
    for pairs in full_assignments(*score.shape):
        total = sum(score[i, j] for i, j in pairs)
        if best is None or total > best_total or (total == best_total and pairs < best):
            best, best_total = pairs, total
    return [(i, j) for i, j in best if score[i, j] > minimum], best_total
