"""A numpy / scipy restatement of the pair boundary census (the tests' reference for rmem_pair_boundary_counts and
rmem_ocu_amd.pairs.pair_boundary_counts), from boolean masks, never through bit planes.

Per frame, with void = (b == void_label) (None: no void): A_i = (a == i) & ~void for i in 1..num_a, B_j = (b == j) & ~void for j in
1..num_b, d = boundary_ref.seg2bmap, (+) r = dilation by the disk dx^2 + dy^2 <= r^2 with zero outside the image:
    bnd_a[i] = |dA_i|, bnd_b[j] = |dB_j|, match[i][j][0] = |dA_i & (dB_j (+) r)|, match[i][j][1] = |dB_j & (dA_i (+) r)|.
Every boundary is dilated once and the pair counts are exact 0 / 1 matrix products.  The dilation is the distance transform's:
a pixel is within the disk of some boundary pixel exactly when its squared Euclidean distance to the nearest one is <= r^2
(boundary_ref.dilate, scipy's binary_dilation with a 127 x 127 disk, takes seconds per mask at r = 63; this takes milliseconds,
and tests/test_pair_boundary_host.py checks that the two agree)."""
import numpy as np
from scipy import ndimage

import boundary_ref


def dilate(b, r):
    """b dilated by the disk of radius r, zero outside the image; an empty b gives an empty result"""
    b = np.asarray(b, dtype=bool)
    if not b.any():
        return np.zeros_like(b)
    d = ndimage.distance_transform_edt(~b)
    return np.rint(d * d).astype(np.int64) <= r * r


def frame_tables(a, b, num_a, num_b, void_label=255, r=1):
    """(match int64 [num_a + 1, num_b + 1, 2], bnd_a int64 [num_a + 1], bnd_b int64 [num_b + 1]) of one frame"""
    a, b = np.asarray(a), np.asarray(b)
    void = np.zeros(b.shape, dtype=bool) if void_label is None else b == void_label
    P = a.size
    ba = np.zeros((num_a + 1, P), dtype=np.int64)
    bb = np.zeros((num_b + 1, P), dtype=np.int64)
    da, db = np.zeros_like(ba), np.zeros_like(bb)
    for i in range(1, num_a + 1):
        m = (a == i) & ~void
        if m.any():
            e = boundary_ref.seg2bmap(m)
            ba[i], da[i] = e.reshape(-1), dilate(e, r).reshape(-1)
    for j in range(1, num_b + 1):
        m = (b == j) & ~void
        if m.any():
            e = boundary_ref.seg2bmap(m)
            bb[j], db[j] = e.reshape(-1), dilate(e, r).reshape(-1)
    match = np.stack([ba @ db.T, da @ bb.T], axis=-1)
    return match, ba.sum(axis=1), bb.sum(axis=1)


def tables(a, b, num_a, num_b, void_label=255, bound_th=0.008):
    """the three tables of a stack [n, H, W]: match [n, num_a + 1, num_b + 1, 2], bnd_a [n, num_a + 1], bnd_b [n, num_b + 1]"""
    a, b = np.asarray(a), np.asarray(b)
    r = boundary_ref.radius(a.shape[1], a.shape[2], bound_th)
    per = [frame_tables(x, y, num_a, num_b, void_label, r) for x, y in zip(a, b)]
    return tuple(np.stack([p[k] for p in per]) for k in range(3))


def f_table(match, bnd_a, bnd_b):
    """F of every pair [n, num_a, num_b], element by element through boundary_ref.f_from_counts"""
    n, na, nb = match.shape[0], match.shape[1] - 1, match.shape[2] - 1
    F = np.zeros((n, na, nb))
    for f in range(n):
        for i in range(na):
            for j in range(nb):
                F[f, i, j] = boundary_ref.f_from_counts(int(bnd_a[f, i + 1]), int(bnd_b[f, j + 1]), int(match[f, i + 1, j + 1, 0]),
                                                        int(match[f, i + 1, j + 1, 1]))
    return F


def unsupervised_brute(J, F, gt_area, gt_bnd, frames=slice(None)):
    """The unsupervised protocol by trying every assignment: J, F [n, num_pred, num_gt] -> (best total of M over one-to-one
    assignments that give every proposal or every object a partner, whichever are fewer; the list of all assignments
    {object: proposal} that reach it within 1e-12)."""
    import itertools
    J, F = np.asarray(J)[frames], np.asarray(F)[frames]
    M = 0.5 * (J.mean(axis=0) + F.mean(axis=0))
    R, C = M.shape
    best, hits = -1.0, []
    if R <= C:
        options = [dict(zip(cols, range(R))) for cols in itertools.permutations(range(C), R)]
    else:
        options = [dict(zip(range(C), rows)) for rows in itertools.permutations(range(R), C)]
    for opt in options:
        total = sum(M[i, j] for j, i in opt.items())
        if total > best + 1e-12:
            best, hits = total, [opt]
        elif abs(total - best) <= 1e-12:
            hits.append(opt)
    return best, hits
