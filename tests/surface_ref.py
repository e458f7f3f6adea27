"""Host restatements of the surface metrics of label stacks (rmem_ocu_amd.surface): numpy, scipy and math.isqrt, nothing of the
product.

surface()        the surface stack by a padded neighbour compare;      surface_erosion()   the same through scipy's binary_erosion;
samples()        the two sample stacks by brute force straight from the definition;
samples_edt()    the same through distance_transform_edt of the complement of the surface mask, squared and rounded;
census()         the table from sorted samples, integer ranks and math.isqrt;
metrics()        hd, hd95, assd and nsd from float roots with np.percentile (linear) and np.mean.
Squared distances are exact integers; SENTINEL = 2^31 - 1 where the other surface is empty."""
import math

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

SENTINEL = 2 ** 31 - 1
EMPTY_ROW = (0, 0, -1, -1, -1, 0, 0, 0, 0)


def _stack(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def surface(labels):
    """uint8 like labels: labels where a 4-neighbour holds another value or lies outside the frame, 0 elsewhere"""
    a = _stack(labels)
    n, H, W = a.shape
    p = np.full((n, H + 2, W + 2), -1, dtype=np.int16)
    p[:, 1:-1, 1:-1] = a
    c = p[:, 1:-1, 1:-1]
    edge = (p[:, :-2, 1:-1] != c) | (p[:, 2:, 1:-1] != c) | (p[:, 1:-1, :-2] != c) | (p[:, 1:-1, 2:] != c)
    return np.where(edge, a, 0).astype(np.uint8).reshape(np.asarray(labels).shape)


def surface_erosion(labels):
    """the same per value: mask & ~binary_erosion(mask, cross, border_value=0)"""
    a = _stack(labels)
    out = np.zeros_like(a)
    cross = generate_binary_structure(2, 1)
    for f in range(a.shape[0]):
        for v in np.unique(a[f]):
            m = a[f] == v
            out[f][m & ~binary_erosion(m, cross, border_value=0)] = v
    return out.reshape(np.asarray(labels).shape)


def _to_mask_brute(mask):
    """int64 [H, W]: the squared distance of every pixel to the nearest True pixel, SENTINEL without one"""
    H, W = mask.shape
    y, x = (c.reshape(-1).astype(np.int64) for c in np.mgrid[0:H, 0:W])
    D = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2
    return np.where(mask.reshape(-1)[None, :], D, SENTINEL).min(axis=1).reshape(H, W)


def _to_mask_edt(mask):
    if not mask.any():
        return np.full(mask.shape, SENTINEL, dtype=np.int64)
    return np.rint(distance_transform_edt(~mask) ** 2).astype(np.int64)


def samples(a, b, num_objs, to_mask=_to_mask_brute):
    """(da, db) int32 like a: da on the surface pixels of object i of a the squared distance to the surface of object i of b, db the
    mirror image; -1 on every other pixel"""
    shape = np.asarray(a).shape
    a, b = _stack(a), _stack(b)
    sa, sb = _stack(surface(a)), _stack(surface(b))
    da, db = np.full(a.shape, -1, dtype=np.int64), np.full(a.shape, -1, dtype=np.int64)
    for f in range(a.shape[0]):
        for i in range(1, num_objs + 1):
            A, B = sa[f] == i, sb[f] == i
            if A.any():
                da[f][A] = to_mask(B)[A]
            if B.any():
                db[f][B] = to_mask(A)[B]
    return da.astype(np.int32).reshape(shape), db.astype(np.int32).reshape(shape)


def samples_edt(a, b, num_objs):
    return samples(a, b, num_objs, _to_mask_edt)


def census_row(values, tol2=(), q=9500):
    """the nine integers of one multiset of samples"""
    s = sorted(int(v) for v in values)
    m = len(s)
    if m == 0:
        return EMPTY_ROW
    if s[0] == SENTINEL:
        assert s[-1] == SENTINEL
        return (m, 0, SENTINEL, SENTINEL, SENTINEL, 0, 0, 0, 0)
    assert s[-1] < 2 ** 30
    pos = (m - 1) * q
    r_lo = pos // 10000
    r_hi = min(r_lo + 1, m - 1)
    within = [sum(1 for v in s if v <= t) for t in tol2] + [0] * (4 - len(tol2))
    return (m, sum(math.isqrt(v << 32) for v in s), s[-1], s[r_lo], s[r_hi], *within)


def census(a, b, num_objs, tol2=(), q=9500, sample_stacks=None):
    """int64 [n, num_objs, 3, 9]"""
    a, b = _stack(a), _stack(b)
    sa, sb = _stack(surface(a)), _stack(surface(b))
    da, db = sample_stacks if sample_stacks is not None else samples_edt(a, b, num_objs)
    da, db = _stack(da), _stack(db)
    n = a.shape[0]
    table = np.zeros((n, num_objs, 3, 9), dtype=np.int64)
    for f in range(n):
        for i in range(1, num_objs + 1):
            s0, s1 = da[f][sa[f] == i].tolist(), db[f][sb[f] == i].tolist()
            for s, vals in enumerate((s0, s1, s0 + s1)):
                table[f, i - 1, s] = census_row(vals, tol2, q)
    return table


def metrics(a, b, num_objs, tolerances=(1.0, 2.0), percentile=95.0, pooled=True):
    """dict of float64 arrays: hd, hd95, assd [n, num_objs] and nsd [n, num_objs, len(tolerances)], from float roots"""
    a, b = _stack(a), _stack(b)
    sa, sb = _stack(surface(a)), _stack(surface(b))
    da, db = (_stack(d) for d in samples_edt(a, b, num_objs))
    n = a.shape[0]
    out = {k: np.zeros((n, num_objs)) for k in ('hd', 'hd95', 'assd')}
    out['nsd'] = np.zeros((n, num_objs, len(tolerances)))
    for f in range(n):
        for i in range(1, num_objs + 1):
            s0, s1 = da[f][sa[f] == i].astype(np.float64), db[f][sb[f] == i].astype(np.float64)
            if s0.size == 0 and s1.size == 0:
                out['nsd'][f, i - 1] = 1.0
                continue
            if s0.size == 0 or s1.size == 0:
                for k in ('hd', 'hd95', 'assd'):
                    out[k][f, i - 1] = np.inf
                continue
            r0, r1 = np.sqrt(s0), np.sqrt(s1)
            r = np.concatenate([r0, r1])
            out['hd'][f, i - 1] = r.max()
            out['hd95'][f, i - 1] = np.percentile(r, percentile) if pooled else max(np.percentile(r0, percentile), np.percentile(r1, percentile))
            out['assd'][f, i - 1] = np.mean(r)
            out['nsd'][f, i - 1] = [np.mean(np.concatenate([s0, s1]) <= math.floor(t * t)) for t in tolerances]
    return out
