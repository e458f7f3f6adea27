"""numpy / pure-Python restatement of the COCO API's run-length masks (maskApi.c: rleEncode, rleToString, rleFrString, rleDecode),
line by line, written independently of rmem_ocu_amd.rle.  Only counts_of is vectorised (np.flatnonzero(np.diff(...))), so that a
480p frame takes milliseconds; the string routines are the C loops."""
import numpy as np


def counts_of(mask):
    """rleEncode: the lengths of the alternating runs of a binary mask [H, W] read column-major, zeros first"""
    m = np.asarray(mask)
    flat = (m != 0).T.reshape(-1)                                  # column-major: position j = x * H + y
    n = flat.size
    edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1      # positions whose value differs from the one before
    bounds = np.concatenate(([0], edges, [n]))
    counts = np.diff(bounds).tolist()
    if n and flat[0]:
        counts = [0] + counts                                      # the first run is of zeros, possibly empty
    return [int(c) for c in counts]


def to_string(counts):
    """rleToString"""
    s = bytearray()
    m = len(counts)
    for i in range(m):
        x = int(counts[i])
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            c += 48
            s.append(c)
    return bytes(s)


def from_string(s):
    """rleFrString"""
    s = bytes(s)
    counts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        m = len(counts)
        if m > 2:
            x += counts[m - 2]
        counts.append(x)
    return counts


def decode(counts, H, W):
    """rleDecode: the binary mask [H, W] (uint8) of a counts list"""
    flat = np.zeros(H * W, dtype=np.uint8)
    at, v = 0, 0
    for c in counts:
        flat[at:at + c] = v
        at += c
        v = 1 - v
    assert at == H * W, (at, H * W)
    return flat.reshape(W, H).T.copy()


def encode_labels(stack, num_ids):
    """[[string of (frame f, id k) for k in 1..num_ids] for f]: what rmem_rle_encode_labels packs, frame-major"""
    stack = np.asarray(stack)
    return [[to_string(counts_of(frame == k)) for k in range(1, num_ids + 1)] for frame in stack]


def paint(frames, H, W):
    """label[mask] = value per frame in listing order: frames[f] = [(value, counts list), ...] -> uint8 [n, H, W]"""
    out = np.zeros((len(frames), H, W), dtype=np.uint8)
    for f, items in enumerate(frames):
        for value, counts in items:
            out[f][decode(counts, H, W) != 0] = value
    return out
