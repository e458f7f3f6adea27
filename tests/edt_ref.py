"""Host restatements of the distance transform of label stacks (rmem_ocu_amd.distance) and of what is built on it.

brute()       both modes straight from the definitions, O(N^2) per frame in numpy: for frames of a few hundred pixels;
edt()         the scipy route for larger ones: per value rint(distance_transform_edt(mask, padded by one pixel if border)^2), with
              the no-site cases handled explicitly (scipy's result there is not a definition);
peaks(), hausdorff2(), next_clicks()
              sequential restatements of the rest.
All squared distances are exact integers (int32); SENTINEL = 2^31 - 1 where there is nothing to measure a distance to."""
import numpy as np
from scipy.ndimage import distance_transform_edt

SENTINEL = 2 ** 31 - 1


def _stack(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def brute(labels, value=None, border=True):
    """int32 like labels: min |p - q|^2 over q with labels[q] != labels[p] (value None; with border the frame's outside joins
    as min(y + 1, H - y, x + 1, W - x)^2), or over q with labels[q] == value; SENTINEL where there is no q"""
    a = _stack(labels)
    n, H, W = a.shape
    y, x = (c.reshape(-1).astype(np.int64) for c in np.mgrid[0:H, 0:W])
    D = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2            # [p, q]
    out = np.empty((n, H * W), dtype=np.int64)
    for f in range(n):
        lab = a[f].reshape(-1)
        if value is None:
            site = lab[None, :] != lab[:, None]
        else:
            site = np.broadcast_to(lab[None, :] == value, D.shape)
        d = np.where(site, D, SENTINEL).min(axis=1)
        if value is None and border:
            d = np.minimum(d, np.minimum(np.minimum(y + 1, H - y), np.minimum(x + 1, W - x)) ** 2)
        out[f] = d
    return out.reshape(np.asarray(labels).shape).astype(np.int32)


def _edt2(mask):
    """squared distance of every True pixel to the nearest False one (0 on False), exact; the mask holds a False pixel"""
    return np.rint(distance_transform_edt(mask) ** 2).astype(np.int64)


def edt(labels, value=None, border=True):
    """the same through scipy"""
    a = _stack(labels)
    n, H, W = a.shape
    out = np.full(a.shape, SENTINEL, dtype=np.int64)
    for f in range(n):
        if value is not None:
            m = a[f] != value
            if not m.all():                                          # else: value is absent, no site
                out[f] = _edt2(m)
            continue
        for v in np.unique(a[f]):
            m = a[f] == v
            if border:
                out[f][m] = _edt2(np.pad(m, 1, constant_values=False))[1:-1, 1:-1][m]
            elif not m.all():                                        # else: a frame of one value, no site
                out[f][m] = _edt2(m)[m]
    return out.reshape(np.asarray(labels).shape).astype(np.int32)


def peaks(dist2, keys):
    """int32 [n, 256, 2]: (largest dist2 among the pixels with keys == v, flat index of the first of them in raster order), (-1, -1)
    for an absent value"""
    d, k = _stack(dist2), _stack(keys)
    n = k.shape[0]
    table = np.full((n, 256, 2), -1, dtype=np.int32)
    for f in range(n):
        df, kf = d[f].reshape(-1), k[f].reshape(-1)
        for p in range(df.size):                                     # sequential: a later pixel wins only if strictly larger
            v = kf[p]
            if df[p] > table[f, v, 0]:
                table[f, v] = (df[p], p)
    return table


def peaks_fast(dist2, keys):
    """peaks() vectorised per value, for frames too large for the sequential walk"""
    d, k = _stack(dist2), _stack(keys)
    n = k.shape[0]
    table = np.full((n, 256, 2), -1, dtype=np.int32)
    for f in range(n):
        df, kf = d[f].reshape(-1), k[f].reshape(-1)
        for v in np.unique(kf):
            idx = np.flatnonzero(kf == v)
            mx = df[idx].max()
            table[f, v] = (mx, idx[np.argmax(df[idx] == mx)])
    return table


def hausdorff2(a, b, num_objs, transform=edt):
    """int32 [n, num_objs]: squared Hausdorff distance of {a == i} and {b == i}; 0 where both are empty, SENTINEL where one is"""
    a, b = _stack(a), _stack(b)
    n = a.shape[0]
    out = np.zeros((n, num_objs), dtype=np.int64)
    for i in range(1, num_objs + 1):
        to_b, to_a = _stack(transform(b, value=i)).astype(np.int64), _stack(transform(a, value=i)).astype(np.int64)
        for f in range(n):
            A, B = a[f] == i, b[f] == i
            if not A.any() and not B.any():
                continue
            if not A.any() or not B.any():
                out[f, i - 1] = SENTINEL
                continue
            out[f, i - 1] = max(to_b[f][A].max(), to_a[f][B].max())
    return out.astype(np.int32)


def next_clicks(pred, gt, num_objs, transform=edt):
    """int32 [n, num_objs, 4]: (y, x, positive, d2) of the deepest point of the deeper error kind (false positive on equal
    depth, first pixel in raster order among equals), (-1, -1, 0, 0) without an error"""
    pred, gt = _stack(pred), _stack(gt)
    n, H, W = pred.shape
    out = np.empty((n, num_objs, 4), dtype=np.int32)
    for i in range(1, num_objs + 1):
        E = np.zeros(pred.shape, dtype=np.uint8)
        E[(gt == i) & (pred != i)] = 1
        E[(pred == i) & (gt != i)] = 2
        d2 = _stack(transform(E, value=None, border=True))
        for f in range(n):
            best = (-1, -1, 0, 0)
            depth = -1
            for kind, positive in ((2, 0), (1, 1)):                  # the false positive first: it wins on equal depth
                m = (E[f] == kind).reshape(-1)
                if not m.any():
                    continue
                df = np.where(m, d2[f].reshape(-1).astype(np.int64), -1)
                mx = int(df.max())
                if mx > depth:
                    p = int(np.argmax(df == mx))
                    depth, best = mx, (p // W, p % W, positive, mx)
            out[f, i - 1] = best
    return out
