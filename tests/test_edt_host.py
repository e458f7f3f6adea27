"""The distance transform's references against each other and against hand-written frames, the workspace sizes, and every refusal
the host makes before anything is launched (no GPU in this tier)."""
import numpy as np
import pytest
import torch

import edt_ref as R

S = R.SENTINEL
HAND = np.array([[0, 0, 1, 1],
                 [0, 0, 1, 1],
                 [0, 0, 0, 0]], dtype=np.uint8)


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    return _lib.lib()


def _cases():
    rng = np.random.default_rng(20)
    for H in range(1, 10):
        for W in range(1, 13):
            nv = 1 + (H + W) % 3
            yield rng.integers(0, nv, (2, H, W)).astype(np.uint8) * 2          # values 0, 2, 4: value 2 is absent when nv == 1
            small = rng.integers(0, 3, (2, (H + 2) // 3, (W + 2) // 3)).astype(np.uint8)
            yield np.kron(small, np.ones((1, 3, 3), dtype=np.uint8))[:, :H, :W]  # 3 x 3-blocky


def test_brute_force_equals_scipy_route():
    count = 0
    for a in _cases():
        for value, border in ((None, False), (None, True), (0, False), (2, False)):
            want, got = R.brute(a, value, border), R.edt(a, value, border)
            assert want.dtype == np.int32 and want.shape == a.shape
            assert np.array_equal(want, got), (a, value, border)
            count += 1
    assert count == 9 * 12 * 2 * 4


def test_a_frame_written_out_by_hand():
    for ref in (R.brute, R.edt):
        assert ref(HAND, None, False).tolist() == [[4, 1, 1, 4], [4, 1, 1, 1], [5, 2, 1, 1]]
        assert ref(HAND, None, True).tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
        assert ref(HAND, 1).tolist() == [[4, 1, 0, 0], [4, 1, 0, 0], [5, 2, 1, 1]]
        assert ref(HAND, 0).tolist() == [[0, 0, 1, 4], [0, 0, 1, 1], [0, 0, 0, 0]]
        assert ref(np.zeros((3, 4), dtype=np.uint8), None, True).tolist() == [[1, 1, 1, 1], [1, 4, 4, 1], [1, 1, 1, 1]]


def test_sentinel_cases():
    one = np.full((2, 3, 4), 9, dtype=np.uint8)
    two = np.stack([HAND, np.zeros_like(HAND)])
    for ref in (R.brute, R.edt):
        assert (ref(one, None, False) == S).all()                    # a frame of one value, no border
        assert (ref(one, 7) == S).all() and (ref(one, 9) == 0).all()
        d = ref(two, 1)                                              # present in the first frame, absent from the next
        assert d[0].max() == 5 and (d[1] == S).all()
        d = ref(two, None, False)
        assert d[0].max() == 5 and (d[1] == S).all()


def test_peaks_hausdorff_and_clicks_restatements():
    rng = np.random.default_rng(21)
    a = rng.integers(0, 4, (2, 7, 9)).astype(np.uint8)
    b = np.roll(a, (1, 2), axis=(1, 2))
    b[1][b[1] == 3] = 0                                              # object 3 absent on one side of frame 1
    d = R.brute(a)
    assert np.array_equal(R.peaks(d, a), R.peaks_fast(d, a)) and np.array_equal(R.peaks(d, b), R.peaks_fast(d, b))
    plateau = np.zeros((3, 4), dtype=np.int32)
    assert R.peaks(plateau, HAND)[0, :3].tolist() == [[0, 0], [0, 2], [-1, -1]]
    h = R.hausdorff2(a, b, 4, R.brute)
    assert np.array_equal(h, R.hausdorff2(a, b, 4, R.edt))
    assert h[1, 2] == S and (h[:, 3] == 0).all() and (R.hausdorff2(a, a, 3) == 0).all()
    assert np.array_equal(R.next_clicks(a, b, 3, R.brute), R.next_clicks(a, b, 3, R.edt))
    gt = np.zeros((1, 5, 7), dtype=np.uint8)
    gt[0, 1:4, 1:4] = 1                                              # a 3 x 3 object; the prediction misses it and puts a 3 x 3 elsewhere
    pred = np.zeros_like(gt)
    assert R.next_clicks(gt, gt, 1).tolist() == [[[-1, -1, 0, 0]]]
    assert R.next_clicks(pred, gt, 1).tolist() == [[[2, 2, 1, 4]]]
    assert R.next_clicks(gt, pred, 1).tolist() == [[[2, 2, 0, 4]]]
    pred[0, 1:4, 4:7] = 1                                            # a false positive of the same depth (the frame's edge at 2): it wins
    assert R.next_clicks(pred, gt, 1).tolist() == [[[2, 5, 0, 4]]]
    pred[:] = 0
    pred[0, 3:5, 4:7] = 1                                            # two rows on the last row: depth 1 everywhere with the border rule
    assert R.next_clicks(pred, gt, 1).tolist() == [[[2, 2, 1, 4]]]
    assert R.next_clicks(pred, np.zeros_like(gt), 1).tolist() == [[[3, 4, 0, 1]]]       # without the rule the peak lay on row 4


def test_workspace_sizes(lib):
    assert lib.rmem_label_edt_workspace_bytes(2, 3, 5) == 64         # 2 * 3 * 5 pixels of 16 bits = 60, in 16-byte units
    assert lib.rmem_label_edt_workspace_bytes(1, 480, 854) == 480 * 854 * 2
    assert lib.rmem_label_edt_workspace_bytes(1, 1, 16384) == 32768 and lib.rmem_label_edt_workspace_bytes(1, 16384, 1) == 32768
    for n, H, W in ((0, 3, 5), (65536, 3, 5), (1, 0, 5), (1, 3, -1), (1, 16385, 1), (1, 1, 16385), (1, 16384, 16384)):
        assert lib.rmem_label_edt_workspace_bytes(n, H, W) == 0, (n, H, W)
    assert lib.rmem_label_edt_peaks_workspace_bytes(3) == 3 * 256 * 8
    assert lib.rmem_label_edt_peaks_workspace_bytes(0) == 0 and lib.rmem_label_edt_peaks_workspace_bytes(65536) == 0


def test_c_entry_points_refuse_on_the_host(lib):
    """non-zero, a message, and nothing launched: the pointers are never looked through"""
    P, n, H, W = 4096, 2, 3, 5                                       # a non-null, aligned address
    need = lib.rmem_label_edt_workspace_bytes(n, H, W)

    def edt(labels=P, n=n, H=H, W=W, value=-1, border=0, dist2=P, ws=P, ws_bytes=need):
        return lib.rmem_label_edt(labels, n, H, W, value, border, dist2, ws, ws_bytes, None)

    for kw, msg in ((dict(labels=None), b'null pointer'), (dict(dist2=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                    (dict(n=0), b'n must be'), (dict(H=0), b'must be positive'), (dict(n=1, H=16385, W=1), b'at most 16384'),
                    (dict(n=1, H=1, W=16385), b'at most 16384'), (dict(n=1, H=16384, W=16384), b'at most 2^26'),
                    (dict(value=256), b'value must be'), (dict(value=-2), b'value must be'), (dict(border=2), b'border must be 0 or 1'),
                    (dict(value=3, border=1), b'border must be 0 with a value'), (dict(ws_bytes=need - 1), b'workspace too small'),
                    (dict(ws=P + 2), b'4-byte aligned')):
        assert edt(**kw) != 0, kw
        assert msg in lib.rmem_last_error_string(), (kw, lib.rmem_last_error_string())
    pneed = lib.rmem_label_edt_peaks_workspace_bytes(n)

    def peaks(dist2=P, keys=P, n=n, H=H, W=W, table=P, ws=P, ws_bytes=pneed):
        return lib.rmem_label_edt_peaks(dist2, keys, n, H, W, table, ws, ws_bytes, None)

    for kw, msg in ((dict(dist2=None), b'null pointer'), (dict(keys=None), b'null pointer'), (dict(table=None), b'null pointer'),
                    (dict(ws=None), b'null pointer'), (dict(n=65536), b'n must be'), (dict(W=0), b'must be positive'),
                    (dict(ws_bytes=pneed - 1), b'workspace too small'), (dict(ws=P + 4), b'8-byte aligned')):
        assert peaks(**kw) != 0, kw
        assert msg in lib.rmem_last_error_string(), (kw, lib.rmem_last_error_string())


def test_python_functions_refuse_on_the_host():
    from rmem_ocu_amd import distance, evaluator
    from rmem_ocu_amd._lib import RmemError
    host = torch.zeros(2, 3, 5, dtype=torch.uint8)
    with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
        distance.label_edt(host)
    with pytest.raises(RmemError, match='labels must be a uint8 device tensor'):
        distance.label_edt(host.int())
    with pytest.raises(RmemError, match='value must be None or an integer in 0..255'):
        distance.label_edt(host, value=256)
    with pytest.raises(RmemError, match='keys must be a uint8 device tensor'):
        distance.peaks(host.int(), host)
    with pytest.raises(RmemError, match='dist2 and keys must have one shape'):
        distance.peaks(torch.zeros(2, 3, 4, dtype=torch.int32), host)
    for fn in (distance.hausdorff2, distance.hausdorff, evaluator.surface_distance, evaluator.next_clicks):
        for bad in (0, 256, 1.5, True):
            with pytest.raises(RmemError, match='num_objs must be an integer in 1..255'):
                fn(host, host, bad)
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host, host, 3)
        with pytest.raises(RmemError, match='must be a uint8 device tensor'):
            fn(host.float(), host.float(), 3)
