"""Host restatements of the nearest-site feature transform of label stacks (rmem_ocu_amd.distance: nearest, grow).

A pixel is a SITE if its value is in `sites`.  Per pixel p of a frame:
  index[p]  the flat index y * W + x of the nearest site by squared Euclidean distance between pixel centres, among equally near
            sites the one with the smallest flat index; -1 where the frame holds no site within max_d2 (-1: no limit; d2 == max_d2
            still counts);
  dist2[p]  that squared distance, SENTINEL = 2^31 - 1 where index is -1;
  taken[p]  labels[index[p]] if labels[p] is in `fill` (None: every value) and index[p] >= 0, else labels[p].

brute()      straight from these lines, O(N^2) per frame: the lexicographic minimum of (d2, index) over all sites;
separable()  the two passes of the device in numpy: per column the nearest site of every row, the one ABOVE on a tie, then per row
             the minimum of (d2, index) over the columns x', one column offset x' - x at a time; O(H W^2), fine up to 1100 columns.
             With bound=True the offsets stop at the root of the frame's largest squared distance as scipy computes it (a column
             farther away than that can neither win nor tie), which is what keeps the device tests quick;
sparse()     the same minimum over an explicit list of sites, O(N S): the closed form for frames with one or two sites, the
             16384-long lines among them.
All return (index int32, dist2 int32, taken uint8) shaped like the labels; the *_keys forms return the minima themselves, int64
[n, H * W] of (d2 << 32) | index (NONE without a site), from which finish() derives the outputs for any `fill` and max_d2.

TIES lists 3 x 3 frames written out by hand: (the sites as (y, x), the pixel, the expected index)."""
import math

import numpy as np
from scipy.ndimage import distance_transform_edt

SENTINEL = 2 ** 31 - 1
NONE = np.iinfo(np.int64).max


def _stack(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def _member(values):
    m = np.zeros(256, dtype=bool)
    if values is None:
        m[:] = True
    else:
        m[np.asarray(sorted(set(int(v) for v in values)), dtype=np.int64)] = True
    return m


def bits(values):
    """the set as eight 32-bit words, bit (v & 31) of word v >> 5"""
    w = [0] * 8
    for v in set(int(v) for v in values):
        w[v >> 5] |= 1 << (v & 31)
    return w


def finish(labels, keys, fill, max_d2):
    """keys int64 [n, HW] = min of (d2 << 32) | index, NONE without a site -> the three outputs"""
    a = _stack(labels)
    n = a.shape[0]
    lab = a.reshape(n, -1)
    found = keys != NONE
    d = np.where(found, keys >> 32, SENTINEL)
    i = np.where(found, keys & 0xffffffff, -1)
    if max_d2 >= 0:
        found &= d <= max_d2
        d, i = np.where(found, d, SENTINEL), np.where(found, i, -1)
    at = np.take_along_axis(lab, np.maximum(i, 0), axis=1)
    taken = np.where(found & _member(fill)[lab], at, lab)
    shape = np.asarray(labels).shape
    return i.astype(np.int32).reshape(shape), d.astype(np.int32).reshape(shape), taken.astype(np.uint8).reshape(shape)


def brute_keys(labels, sites):
    a = _stack(labels)
    n, H, W = a.shape
    y, x = (c.reshape(-1).astype(np.int64) for c in np.mgrid[0:H, 0:W])
    key = (((y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2) << 32) | np.arange(H * W, dtype=np.int64)[None, :]   # [p, q]
    is_site = _member(sites)
    keys = np.empty((n, H * W), dtype=np.int64)
    for f in range(n):
        site = is_site[a[f].reshape(-1)]
        keys[f] = np.where(site[None, :], key, NONE).min(axis=1)
    return keys


def brute(labels, sites, fill=None, max_d2=-1):
    return finish(labels, brute_keys(labels, sites), fill, max_d2)


def column_candidates(site):
    """site bool [H, W] -> int64 [H, W]: the row of the nearest site of every pixel's own column, the one above on a tie, -1 where
    the column holds none"""
    H, W = site.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(site, rows, -1), axis=0)
    below = np.minimum.accumulate(np.where(site, rows, 2 * H)[::-1], axis=0)[::-1]
    take_above = (above >= 0) & ((below == 2 * H) | (rows - above <= below - rows))
    return np.where(take_above, above, np.where(below == 2 * H, -1, below))


def separable_keys(labels, sites, bound=False):
    a = _stack(labels)
    n, H, W = a.shape
    is_site = _member(sites)
    rows, cols = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    keys = np.full((n, H, W), NONE, dtype=np.int64)
    for f in range(n):
        site = is_site[a[f]]
        if not site.any():
            continue
        reach = W - 1
        if bound:
            reach = min(reach, math.isqrt(int(np.rint(distance_transform_edt(~site).max() ** 2))))
        cand = column_candidates(site)
        own = np.where(cand >= 0, (((cand - rows) ** 2) << 32) | (cand * W + cols), NONE)   # the key of a column's candidate at dx = 0
        for dx in range(-reach, reach + 1):                          # the pixel at x looks at column x + dx
            lo, hi = max(0, -dx), min(W, W - dx)
            there = own[:, lo + dx:hi + dx]
            k = np.where(there != NONE, there + (dx * dx << 32), NONE)
            keys[f, :, lo:hi] = np.minimum(keys[f, :, lo:hi], k)
    return keys.reshape(n, -1)


def separable(labels, sites, fill=None, max_d2=-1, bound=False):
    return finish(labels, separable_keys(labels, sites, bound), fill, max_d2)


def sparse_keys(labels, sites):
    a = _stack(labels)
    n, H, W = a.shape
    is_site = _member(sites)
    p = np.arange(H * W, dtype=np.int64)
    py, px = p // W, p % W
    keys = np.full((n, H * W), NONE, dtype=np.int64)
    for f in range(n):
        for q in np.flatnonzero(is_site[a[f].reshape(-1)]):
            keys[f] = np.minimum(keys[f], (((py - q // W) ** 2 + (px - q % W) ** 2) << 32) | q)
    return keys


def sparse(labels, sites, fill=None, max_d2=-1):
    return finish(labels, sparse_keys(labels, sites), fill, max_d2)


CORNERS = ((0, 0), (0, 2), (2, 0), (2, 2))
TIES = ((CORNERS, (1, 1), 0),
        (CORNERS, (1, 0), 0),                                        # above beats below
        (CORNERS, (1, 2), 2),
        (CORNERS, (2, 1), 6),
        (((0, 2), (2, 0)), (1, 1), 2),
        (((1, 0), (0, 1)), (1, 1), 1),
        (((1, 0), (1, 2)), (1, 1), 3),
        (((1, 0), (0, 1)), (0, 0), 1))                               # the same-row site at dx^2 == best beats the own column's site below


def tie_frame(sites_at, shape=(3, 3), at=(0, 0), value=3):
    """a frame of zeros with `value` at the given pixels, moved by `at`"""
    a = np.zeros(shape, dtype=np.uint8)
    for y, x in sites_at:
        a[y + at[0], x + at[1]] = value
    return a
