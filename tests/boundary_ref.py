"""A numpy restatement of the DAVIS boundary measure F and region measure J (the tests' reference for rmem_clip_score_counts and
rmem_ocu_amd.evaluator.score_clip).

Follows the published evaluation code: seg2bmap at the mask's own size, a disk structuring element dx^2 + dy^2 <= r^2 (skimage's
disk), dilation with zero padding (done here by scipy.ndimage.binary_dilation), f_measure's precision / recall edge cases,
db_eval_iou, and db_statistics (mean, recall, decay).  Slow: about 0.4 s per object and 480p frame.
"""
import math

import numpy as np
from scipy import ndimage


def radius(H, W, bound_th=0.008):
    return int(bound_th) if bound_th >= 1 else int(math.ceil(bound_th * math.sqrt(H * H + W * W)))


def seg2bmap(seg):
    seg = np.asarray(seg).astype(bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def disk(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (xx * xx + yy * yy) <= r * r


def dilate(b, r):
    return ndimage.binary_dilation(b, structure=disk(r), border_value=0)


def dilate_brute(b, r):
    """the definition, pixel by pixel: out[y, x] = any b[y + dy, x + dx] with dx^2 + dy^2 <= r^2 inside the image"""
    H, W = b.shape
    out = np.zeros_like(b, dtype=bool)
    for y, x in zip(*np.nonzero(b)):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx * dx + dy * dy <= r * r and 0 <= y + dy < H and 0 <= x + dx < W:
                    out[y + dy, x + dx] = True
    return out


def frame_counts(pred, gt, num_ids, void_label=255, bound_th=0.008):
    """[num_ids, 6] int64 for one frame: n_fg, n_gt, fg_match, gt_match, J intersection, J union (row 0 zero)"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    r = radius(pred.shape[0], pred.shape[1], bound_th)
    void = gt == void_label
    out = np.zeros((num_ids, 6), dtype=np.int64)
    for k in range(1, num_ids):
        fm, gm = (pred == k) & ~void, (gt == k) & ~void
        out[k, 4], out[k, 5] = (fm & gm).sum(), (fm | gm).sum()
        fb, gb = seg2bmap(fm), seg2bmap(gm)
        out[k, 0], out[k, 1] = fb.sum(), gb.sum()
        if out[k, 0] and out[k, 1]:
            out[k, 2] = (fb & dilate(gb, r)).sum()
            out[k, 3] = (gb & dilate(fb, r)).sum()
    return out


def clip_counts(pred, gt, num_ids, void_label=255, bound_th=0.008):
    return np.stack([frame_counts(p, g, num_ids, void_label, bound_th) for p, g in zip(pred, gt)])


def f_from_counts(n_fg, n_gt, fg_match, gt_match):
    """f_measure's last lines, scalar"""
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = fg_match / float(n_fg), gt_match / float(n_gt)
    return 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)


def j_from_counts(inter, union):
    return 1.0 if union == 0 else inter / float(union)


def scores(counts):
    """counts [n, num_ids, 6] -> (J, F) [n, num_ids], element by element"""
    counts = np.asarray(counts)
    J = np.zeros(counts.shape[:2])
    F = np.zeros(counts.shape[:2])
    for t in range(counts.shape[0]):
        for k in range(counts.shape[1]):
            c = [int(v) for v in counts[t, k]]
            J[t, k] = j_from_counts(c[4], c[5])
            F[t, k] = f_from_counts(c[0], c[1], c[2], c[3])
    return J, F


def db_statistics(values):
    """mean, recall and decay of one object's per-frame values (no NaN here: every frame is scored)"""
    values = np.asarray(values, dtype=np.float64)
    M = np.mean(values)
    O = np.mean(values > 0.5)
    ids = np.round(np.linspace(1, len(values), 5) + 1e-10) - 1
    ids = ids.astype(np.int64)
    bins = [values[ids[i]:ids[i + 1] + 1] for i in range(4)]
    D = np.mean(bins[0]) - np.mean(bins[3])
    return M, O, D


def summary(J, F, frames=slice(1, -1), tail=0.25):
    """J, F [n, num_objs] -> dict of the clip summary: per object mean / recall / decay over the selected frames, their means
    over objects, J&F, and the tail J (frames int(len * (1 - tail)) .. end of the selection)."""
    J, F = np.asarray(J)[frames], np.asarray(F)[frames]
    nobj = J.shape[1]
    js = np.array([db_statistics(J[:, o]) for o in range(nobj)])
    fs = np.array([db_statistics(F[:, o]) for o in range(nobj)])
    start = int(J.shape[0] * (1.0 - tail))
    jt = np.array([np.mean(J[start:, o]) for o in range(nobj)])
    return dict(J_obj_mean=js[:, 0], J_obj_recall=js[:, 1], J_obj_decay=js[:, 2], F_obj_mean=fs[:, 0], F_obj_recall=fs[:, 1],
                F_obj_decay=fs[:, 2], J_obj_tail=jt, J_mean=js[:, 0].mean(), J_recall=js[:, 1].mean(), J_decay=js[:, 2].mean(),
                F_mean=fs[:, 0].mean(), F_recall=fs[:, 1].mean(), F_decay=fs[:, 2].mean(),
                JF_mean=(js[:, 0].mean() + fs[:, 0].mean()) / 2.0, J_tail=jt.mean())


def blobs(H, W, n_ids=5, seed=0):
    """a seeded label map: n_ids - 1 overlapping ellipses (ids 1..n_ids-1) on background"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), dtype=np.uint8)
    for k in range(1, n_ids):
        cy, cx = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W
        ry, rx = rs.uniform(0.12, 0.3) * H, rs.uniform(0.12, 0.3) * W
        lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    return lab


def shifted_speckled(lab, dy, dx, seed=0, speckles=40):
    """`lab` moved by (dy, dx) (background moves in), then `speckles` random pixels relabelled"""
    H, W = lab.shape
    out = np.zeros_like(lab)
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[yd, xd] = lab[ys, xs]
    rs = np.random.RandomState(seed + 1000)
    n_ids = int(lab.max()) + 1
    out[rs.randint(0, H, speckles), rs.randint(0, W, speckles)] = rs.randint(0, n_ids, speckles)
    return out
