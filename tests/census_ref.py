"""numpy restatement of the label census, the clip protocol rule, its tables and overlays, and the per-object score summary:
written from include/rmem.h and the reference's dataset class (dataloaders/eval_datasets.py, VOSTest), independently of
rmem_ocu_amd.protocol.  The protocol rule works on the label maps directly (np.unique per frame), never through the census."""
import numpy as np


def census(labels):
    """int32 [n, 256, 5] = area, xmin, ymin, xmax, ymax per frame and value; (0, W, H, -1, -1) for an absent value."""
    labels = np.asarray(labels)
    n, H, W = labels.shape
    out = np.empty((n, 256, 5), dtype=np.int32)
    out[:] = (0, W, H, -1, -1)
    for f in range(n):
        for v in np.unique(labels[f]):
            ys, xs = np.nonzero(labels[f] == v)
            out[f, int(v)] = (ys.size, xs.min(), ys.min(), xs.max(), ys.max())
    return out


def protocol(labels, frame_index=None, void_label=255):
    """The curr_objs loop of VOSTest on the label maps -> (squeeze_idx, first_frame, new_frames)."""
    labels = np.asarray(labels)
    frame_index = list(range(labels.shape[0])) if frame_index is None else list(frame_index)
    curr_objs, first_frame = [0], []
    for label, t in zip(labels, frame_index):
        for v in np.unique(label):                                 # ascending
            v = int(v)
            if v == void_label or v in curr_objs:
                continue
            curr_objs.append(v)
            first_frame.append(t)
    new_frames = sorted(set(t for t in first_frame if t > 0))
    return curr_objs, first_frame, new_frames


def tables(squeeze_idx, first_frame, void_label=255):
    """(lut_all, lut_first, {t: lut_new[t]}) uint8 [256] each."""
    lut_all = np.zeros(256, dtype=np.uint8)
    lut_first = np.zeros(256, dtype=np.uint8)
    lut_new = {}
    for k in range(1, len(squeeze_idx)):
        t = first_frame[k - 1]
        lut_all[squeeze_idx[k]] = k
        if t == 0:
            lut_first[squeeze_idx[k]] = k
        else:
            lut_new.setdefault(t, np.zeros(256, dtype=np.uint8))[squeeze_idx[k]] = k
    if void_label is not None:
        lut_all[void_label] = void_label
    return lut_all, lut_first, lut_new


def overlays(labels, frame_index=None, void_label=255):
    """(first label, {t: overlay}) in squeezed ids, built pixel set by pixel set: the first label holds the objects of frame 0, an
    overlay only the objects that first appear on its frame."""
    labels = np.asarray(labels)
    frame_index = list(range(labels.shape[0])) if frame_index is None else list(frame_index)
    squeeze_idx, first_frame, new_frames = protocol(labels, frame_index, void_label)
    first = np.zeros(labels.shape[1:], dtype=np.uint8)
    new = {t: np.zeros(labels.shape[1:], dtype=np.uint8) for t in new_frames}
    for k in range(1, len(squeeze_idx)):
        t = first_frame[k - 1]
        row = frame_index.index(t)
        (first if t == 0 else new[t])[labels[row] == squeeze_idx[k]] = k
    return first, new


def _statistics(v):
    """db_statistics of the benchmark toolkit: mean, recall (> 0.5), decay over four bins."""
    v = np.asarray(v, dtype=np.float64)
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.int64)
    b0, b3 = v[ids[0]:ids[1] + 1], v[ids[3]:ids[4] + 1]
    return np.mean(v), np.mean(v > 0.5), np.mean(b0) - np.mean(b3)


def per_object_summary(J, F, first_frames, tail=0.25):
    """Object k (column k - 1) over frames first_frames[k - 1] + 1 .. n - 2 -> dict of per-object arrays and their means."""
    J, F = np.asarray(J, dtype=np.float64), np.asarray(F, dtype=np.float64)
    n = J.shape[0]
    keys = ('J_obj_mean', 'J_obj_recall', 'J_obj_decay', 'F_obj_mean', 'F_obj_recall', 'F_obj_decay', 'J_obj_tail')
    out = {k: [] for k in keys}
    frames = []
    for o, t in enumerate(first_frames):
        sel = np.arange(int(t) + 1, n - 1)
        frames.append(sel)
        for name, v in (('J', J[sel, o]), ('F', F[sel, o])):
            mean, recall, decay = _statistics(v)
            out[f'{name}_obj_mean'].append(mean)
            out[f'{name}_obj_recall'].append(recall)
            out[f'{name}_obj_decay'].append(decay)
        out['J_obj_tail'].append(np.mean(J[sel[int(sel.size * (1.0 - tail)):], o]))
    out = {k: np.array(v) for k, v in out.items()}
    out.update(J_mean=float(out['J_obj_mean'].mean()), J_recall=float(out['J_obj_recall'].mean()), J_decay=float(out['J_obj_decay'].mean()),
               F_mean=float(out['F_obj_mean'].mean()), F_recall=float(out['F_obj_recall'].mean()), F_decay=float(out['F_obj_decay'].mean()),
               JF_mean=float(0.5 * (out['J_obj_mean'].mean() + out['F_obj_mean'].mean())), J_tail=float(out['J_obj_tail'].mean()))
    out['obj_frames'] = frames
    return out


SCORE_FIELDS = ('J_obj_mean', 'J_obj_recall', 'J_obj_decay', 'F_obj_mean', 'F_obj_recall', 'F_obj_decay', 'J_obj_tail', 'J_mean',
                'J_recall', 'J_decay', 'F_mean', 'F_recall', 'F_decay', 'JF_mean', 'J_tail')


def assert_score_equals(score, want):
    """every summary field of a ClipScore equals per_object_summary's, exactly"""
    for k in SCORE_FIELDS:
        assert np.array_equal(np.asarray(getattr(score, k)), np.asarray(want[k])), k
    assert len(score.obj_frames) == len(want['obj_frames'])
    for a, b in zip(score.obj_frames, want['obj_frames']):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- contents
def blobs(seed, n, H, W, ids=tuple(range(1, 11))):
    """seeded rectangles of the given ids on background 0, drifting from frame to frame"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, H, W), dtype=np.uint8)
    for v in ids:
        h, w = int(rng.integers(1, max(H // 3, 2))), int(rng.integers(1, max(W // 3, 2)))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        for f in range(n):
            yy, xx = min(y + f, H - h), min(x + 2 * f, W - w)
            a[f, yy:yy + h, xx:xx + w] = v
    return a
