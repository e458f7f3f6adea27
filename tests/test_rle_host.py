"""COCO run-length masks, the part that needs no GPU: the reference (tests/rle_ref.py) pinned to literal vectors, the host helpers
of rmem_ocu_amd.rle against it, the transition property the device encoder is built on, the layout of PackedRles, and every
host-side refusal of the C entry points."""
import os

import numpy as np
import pytest

import rle_ref


def _mask(H, W, *boxes):
    m = np.zeros((H, W), dtype=np.uint8)
    for ys, xs in boxes:
        m[ys, xs] = 1
    return m


VECTORS = [
    (_mask(3, 4, (slice(1, 3), slice(1, 3))), [4, 2, 1, 2, 3], b'42102'),                   # the third count is not delta'd
    (_mask(5, 7, (0, 0)), [0, 1, 34], b'01R1'),
    (_mask(5, 7, (4, 6)), [34, 1], b'R11'),
    (np.zeros((480, 854), dtype=np.uint8), [480 * 854], b'PZ`<'),
    (np.ones((480, 854), dtype=np.uint8), [0, 480 * 854], b'0PZ`<'),
    (_mask(40, 3, (slice(2, 39), 0), (slice(0, 3), 1), (39, 2)), [2, 37, 1, 3, 76, 1], b'2U11nN[2N'),   # negative deltas
]


@pytest.mark.parametrize('k', range(len(VECTORS)))
def test_reference_matches_the_literal_vectors(k):
    mask, counts, string = VECTORS[k]
    assert rle_ref.counts_of(mask) == counts
    assert rle_ref.to_string(counts) == string
    assert rle_ref.from_string(string) == counts
    assert np.array_equal(rle_ref.decode(counts, *mask.shape), mask)


def test_reference_matches_pycocotools_when_installed():
    mask_api = pytest.importorskip('pycocotools.mask')
    rng = np.random.default_rng(3)
    masks = [v[0] for v in VECTORS] + [(rng.random((37, 53)) < p).astype(np.uint8) for p in (0.02, 0.5, 0.98)]
    for m in masks:
        r = mask_api.encode(np.asfortranarray(m))
        assert r['counts'] == rle_ref.to_string(rle_ref.counts_of(m)) and list(r['size']) == list(m.shape)
        assert np.array_equal(mask_api.decode(r), m)


def _random_masks():
    rng = np.random.default_rng(11)
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 5), (33, 18)):
        for p in (0.0, 0.1, 0.5, 0.9, 1.0):
            yield (rng.random((H, W)) < p).astype(np.uint8)


def test_reference_round_trips():
    for m in _random_masks():
        c = rle_ref.counts_of(m)
        assert sum(c) == m.size and all(v > 0 for v in c[1:]) and c[0] >= 0
        assert rle_ref.from_string(rle_ref.to_string(c)) == c
        assert np.array_equal(rle_ref.decode(c, *m.shape), m)
        assert all(48 <= b <= 111 for b in rle_ref.to_string(c))


def test_string_from_counts_equals_the_reference():
    from rmem_ocu_amd import rle
    for _, counts, string in VECTORS:
        assert rle.string_from_counts(counts) == string
    for m in _random_masks():
        c = rle_ref.counts_of(m)
        assert rle.string_from_counts(c) == rle_ref.to_string(c)
    big = [0, 1 << 26] + [3, (1 << 26) - 7, 5, 1, 1 << 20]            # six characters, and deltas of both signs
    assert rle.string_from_counts(big) == rle_ref.to_string(big) and rle_ref.from_string(rle_ref.to_string(big)) == big


def test_run_boundaries_are_the_label_transitions():
    """For a label map the boundaries of all objects together are the label transitions in column-major order with
    label[-1] := 0; object k's counts are the differences of its boundary positions, closed by H * W."""
    rng = np.random.default_rng(5)
    for H, W, K in ((1, 1, 1), (1, 7, 2), (6, 1, 3), (5, 7, 3), (16, 9, 4)):
        for hi in (K, K + 2):                                            # values above K belong to no mask
            for _ in range(20):
                lab = rng.integers(0, hi + 1, (H, W))
                flat = np.where(lab > K, 0, lab).T.reshape(-1)
                bounds = {k: [] for k in range(1, K + 1)}
                prev = 0
                for j, v in enumerate(flat.tolist()):
                    if v != prev:
                        if prev:
                            bounds[prev].append(j)
                        if v:
                            bounds[v].append(j)
                        prev = v
                for k in range(1, K + 1):
                    b = [0] + bounds[k] + [H * W]
                    assert [q - p for p, q in zip(b, b[1:])] == rle_ref.counts_of(lab == k), (H, W, k)


def test_packed_rles_layout():
    from rmem_ocu_amd import _lib, rle
    H, W = 5, 7
    m1, m2 = _mask(H, W, (slice(0, 2), slice(0, 3))), _mask(H, W, (4, 6))
    r1 = {'size': [H, W], 'counts': rle_ref.to_string(rle_ref.counts_of(m1))}
    r2 = {'size': [H, W], 'counts': rle_ref.to_string(rle_ref.counts_of(m2)).decode()}
    r3 = {'size': [H, W], 'counts': rle_ref.counts_of(m1)}             # the uncompressed form
    p = rle.PackedRles([{3: r1, 9: r2}, [], [(200, r3), (1, r2)]], (H, W))
    assert len(p) == 4 and tuple(p.shape) == (3, H, W)
    strings = [r1['counts'], r2['counts'].encode(), r1['counts'], r2['counts'].encode()]
    assert bytes(p.buf.numpy().tobytes()) == b''.join(strings) and p.total_bytes == sum(map(len, strings))
    got = [(d.frame, d.value, d.offset, d.length) for d in p.descs]
    at, want = 0, []
    for (f, v), s in zip([(0, 3), (0, 9), (2, 200), (2, 1)], strings):
        want.append((f, v, at, len(s)))
        at += len(s)
    assert got == want
    import ctypes
    assert ctypes.sizeof(_lib.RleDesc) == 24 and p.desc_bytes.numel() == 4 * 24
    assert p.NOUN and set(p.STATUS_NAMES) == {1, 2, 4, 8, 16, 32}


def test_packed_rles_refusals():
    from rmem_ocu_amd import rle
    from rmem_ocu_amd._lib import RmemError
    from rmem_ocu_amd.evaluator import labels_from_rles
    good = {'size': [5, 7], 'counts': b'R11'}
    with pytest.raises(RmemError, match='size'):
        rle.PackedRles([{1: good}], (7, 5))
    with pytest.raises(RmemError, match='size'):
        rle.PackedRles([{1: good}, {1: {'size': [5, 8], 'counts': b'R11'}}], (5, 7))
    with pytest.raises(RmemError, match='1..255'):
        rle.PackedRles([{256: good}], (5, 7))
    with pytest.raises(RmemError, match='1..255'):
        rle.PackedRles([{0: good}], (5, 7))
    with pytest.raises(RmemError, match='255'):
        rle.PackedRles([[(1, good)] * 256], (5, 7))
    with pytest.raises(RmemError, match='counts'):
        rle.PackedRles([{1: b'R11'}], (5, 7))
    with pytest.raises(RmemError, match='256 tracks'):
        labels_from_rles([{t: good for t in range(256)}], (5, 7), 'cuda')          # refused before any device is touched
    with pytest.raises(RmemError, match='GPU device'):
        rle.decode_label_stack([{1: good}], (5, 7), 'cpu')


def test_argument_validation_needs_no_gpu():
    """Every refusal of the two entry points and the two workspace functions happens on the host, with a message."""
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    P = 64                                                               # a non-null, 16-byte aligned address that is never used

    def enc(labels=P, n=1, H=4, W=4, K=1, ws=P, out=P, cap=16, offsets=P, status=P):
        return L.rmem_rle_encode_labels(labels, n, H, W, K, ws, out, cap, offsets, status, None)

    def dec(bits=P, total=8, descs=P, ns=1, n=1, H=4, W=4, ws=P, labels=P, status=P):
        return L.rmem_rle_decode_labels(bits, total, descs, ns, n, H, W, ws, labels, status, None)

    def refused(rc, text):
        assert rc != 0 and text in L.rmem_last_error_string(), (rc, L.rmem_last_error_string())

    for name in ('labels', 'ws', 'out', 'offsets', 'status'):
        refused(enc(**{name: None}), b'null pointer')
    refused(enc(n=0), b'frames')
    refused(enc(n=65536), b'frames')
    refused(enc(H=0), b'H and W')
    refused(enc(W=-1), b'H and W')
    refused(enc(H=8193, W=8192), b'2^26')
    refused(enc(K=0), b'num_ids')
    refused(enc(K=256), b'num_ids')
    refused(enc(cap=-1), b'capacity')
    refused(enc(ws=P + 4), b'aligned')
    for name in ('bits', 'descs', 'ws', 'labels', 'status'):
        refused(dec(**{name: None}), b'null pointer')
    refused(dec(total=-1), b'total_bytes')
    refused(dec(total=1 << 31), b'total_bytes')
    refused(dec(ns=0), b'nstrings')
    refused(dec(n=0), b'frames')
    refused(dec(n=65536), b'frames')
    refused(dec(H=0), b'H and W')
    refused(dec(H=8193, W=8192), b'2^26')
    refused(dec(ws=P + 8), b'aligned')
    W = L.rmem_rle_workspace_bytes
    assert W(0, 4, 4, 1) == 0 and W(65536, 4, 4, 1) == 0 and W(1, 0, 4, 1) == 0 and W(1, 8193, 8192, 1) == 0
    assert W(1, 4, 4, 0) == 0 and W(1, 4, 4, 256) == 0
    assert W(1, 480, 854, 10) >= 8 * 480 * 854 + 4 * 10 * 854 * 4 and W(2, 480, 854, 10) <= 2 * W(1, 480, 854, 10)
    assert W(1, 8192, 8192, 255) > 0
    D = L.rmem_rle_decode_workspace_bytes
    assert D(0, 8, 1, 4) == 0 and D(1, -1, 1, 4) == 0 and D(1, 1 << 31, 1, 4) == 0 and D(1, 8, 0, 4) == 0 and D(1, 8, 65536, 4) == 0
    assert D(1, 8, 1, 0) == 0 and D(1, 8, 1, (1 << 26) + 1) == 0
    assert D(3, 100, 2, 7) >= 4 * 100 + (16 + 4 * 7) * 3 + 8 * 2 and D(1, 0, 1, 1) > 0
