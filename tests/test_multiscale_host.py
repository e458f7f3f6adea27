"""Host side of multi-scale testing inside clip groups: the symbol and its binding, the refusals that need no GPU, the slot's
constructor checks, and a replay of the tile kernel's index arithmetic (k_logits_ms_merge_tile, resample.hip) in Python."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

FP_H, FP_W, FP_SRC = 16, 32, 192          # resample.hip


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbol_is_exported_and_bound_at_abi_15(lib):
    from rmem_ocu_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'rmem.h')).read()
    assert re.search(r'#define\s+RMEM_ABI_VERSION\s+15\b', header) and 'rmem_logits_post_ms_merge' in header
    assert _lib.ABI_VERSION == 15 and lib.rmem_abi_version() == 15
    assert 'rmem_logits_post_ms_merge' in _lib.SIGNATURES and hasattr(lib, 'rmem_logits_post_ms_merge')
    assert callable(ops.logits_post_ms_merge)


def _call(lib, members, his, wis, flips, n_aug, P, nc, keep, Ho, Wo, label, twin=None):
    n = max(len(members), 1)
    arr = (C.c_void_p * n)(*members)
    return lib.rmem_logits_post_ms_merge(arr, (C.c_int * n)(*his), (C.c_int * n)(*wis), (C.c_int * n)(*flips), n_aug, P, nc, keep, Ho, Wo, 1,
                                         label, twin, None)


def test_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    """Every refusal of include/rmem.h, on the host, before anything is launched (the pointers are never dereferenced)."""
    err = lib.rmem_last_error_string
    two = dict(members=[4096, 8192], his=[9, 13], wis=[11, 15], flips=[0, 1])

    def call(n_aug=2, P=2, nc=11, keep=6, Ho=40, Wo=50, label=4096, **over):
        a = dict(two, **over)
        return _call(lib, a['members'], a['his'], a['wis'], a['flips'], n_aug, P, nc, keep, Ho, Wo, label)

    assert call(n_aug=0) != 0 and b'1..8 members' in err()
    assert _call(lib, [4096] * 9, [9] * 9, [11] * 9, [0] * 9, 9, 2, 11, 6, 40, 50, 4096) != 0 and b'1..8 members' in err()
    assert call(nc=17) != 0 and b'classes' in err()
    assert call(keep=11) != 0 and b'keep_max_id' in err()
    assert call(P=0) != 0 and b'clips' in err()
    assert call(Ho=0) != 0 and b'size' in err()
    assert call(Wo=-3) != 0 and b'size' in err()
    assert call(his=[9, 0]) != 0 and b'size' in err()
    assert call(wis=[-1, 15]) != 0 and b'size' in err()
    assert call(members=[4096, None]) != 0 and b'null' in err()
    assert call(label=None) != 0 and b'null' in err()
    assert call(members=[4096, 8192 + 4]) != 0 and b'16-byte' in err()


def test_op_refuses_before_touching_the_device():
    from rmem_ocu_amd import ops
    from rmem_ocu_amd._lib import RmemError
    lg = torch.zeros(2, 9 * 11, 16)
    lab = torch.zeros(2, 33, 43, dtype=torch.uint8)
    one = (lg, 9, 11, False)
    with pytest.raises(RmemError, match='members'):
        ops.logits_post_ms_merge([], 11, 6, 33, 43, True, lab, P=2)
    with pytest.raises(RmemError, match='members'):
        ops.logits_post_ms_merge([one] * 9, 11, 6, 33, 43, True, lab, P=2)
    with pytest.raises(RmemError, match='keep'):
        ops.logits_post_ms_merge([one], 11, 11, 33, 43, True, lab, P=2)
    with pytest.raises(RmemError, match='clip'):
        ops.logits_post_ms_merge([one], 11, 6, 33, 43, True, lab, P=0)
    with pytest.raises(RmemError, match='device tensors'):          # and, as every op, no CPU fallback
        ops.logits_post_ms_merge([one], 11, 6, 33, 43, True, lab, P=2)


class _StubEngine:
    def __init__(self, rows=4, flip=False, lookahead=4, device='cpu'):
        self.B, self.flip_tta, self.lookahead, self.device = rows, flip, lookahead, device

    def propagate_to_logits(self, enc_slot=None, imgs=None):
        raise AssertionError('the constructor runs nothing')


def test_slot_constructor_refuses_mismatched_engines_by_name():
    from rmem_ocu_amd.clip_runner import MultiScaleGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from rmem_ocu_amd import evaluator
    assert callable(GroupEngine.propagate_to_logits) and callable(evaluator.run_group_multiscale)
    E = _StubEngine
    with pytest.raises(ValueError, match='rows'):
        MultiScaleGroupSlot([E(4), E(6)], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='flip_tta'):
        MultiScaleGroupSlot([E(4, True), E(4, False)], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='lookahead'):
        MultiScaleGroupSlot([E(4), E(4, lookahead=1)], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='device'):
        MultiScaleGroupSlot([E(4), E(4, device='meta')], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='at most 8'):
        MultiScaleGroupSlot([E(4, True) for _ in range(5)], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='at most 8'):
        MultiScaleGroupSlot([E(4) for _ in range(9)], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='RaggedGroupSlot'):
        MultiScaleGroupSlot([object()], (40, 50), 'cpu')
    with pytest.raises(ValueError, match='at least one'):
        MultiScaleGroupSlot([], (40, 50), 'cpu')


# ------------------------------------------------------------------------------------------------- the tile route's indices
@functools.lru_cache(maxsize=None)
def src_coord(d, n_in, n_out, align):
    """rmem_src_coord (csrc/common.h) in float32: -> (i0, i1); the weight does not enter the index arithmetic"""
    f = np.float32
    if align:
        s = f(d) * (f(n_in - 1) / f(n_out - 1)) if n_out > 1 else f(0)
    else:
        # fmaf((float)d + 0.5f, (float)in / (float)out, -0.5f): one rounding (the float64 product of two float32 is exact)
        s = max(f(np.float64(f(d) + f(0.5)) * np.float64(f(n_in) / f(n_out)) - 0.5), f(0))
    i0 = min(int(s), n_in - 1)
    return i0, min(i0 + 1, n_in - 1)


def replay_taps(members, Ho, Wo, align):
    """The staging and the taps of k_logits_ms_merge_tile thread by thread for one clip -> the largest staged extent in pixels;
    asserts that the staging loads stay inside the member and every tap inside its member's stage."""
    worst = 0
    tiles_x = (Wo + FP_W - 1) // FP_W
    for blk in range(((Ho + FP_H - 1) // FP_H) * tiles_x):
        ty, tx = divmod(blk, tiles_x)
        oy0, ox0 = ty * FP_H, tx * FP_W
        oy1, ox1 = min(oy0 + FP_H, Ho) - 1, min(ox0 + FP_W, Wo) - 1
        for Hi, Wi, fl in members:
            c0, c1 = (Wo - 1 - ox1, Wo - 1 - ox0) if fl else (ox0, ox1)
            ylo, yhi = src_coord(oy0, Hi, Ho, align)[0], src_coord(oy1, Hi, Ho, align)[1]
            xlo, xhi = src_coord(c0, Wi, Wo, align)[0], src_coord(c1, Wi, Wo, align)[1]
            nrows, ncols = yhi - ylo + 1, xhi - xlo + 1
            assert nrows >= 1 and ncols >= 1 and 0 <= ylo and yhi < Hi and 0 <= xlo and xhi < Wi
            worst = max(worst, nrows * ncols)
            for t in range(128):
                oy, oxb = oy0 + (t >> 3), ox0 + (t & 7) * 4
                if oy >= Ho or oxb >= Wo:
                    continue
                y0, y1 = src_coord(oy, Hi, Ho, align)
                assert 0 <= y0 - ylo <= y1 - ylo < nrows, (blk, t, (Hi, Wi, fl))
                for ox in range(oxb, min(oxb + 4, Wo)):
                    x0, x1 = src_coord(Wo - 1 - ox if fl else ox, Wi, Wo, align)
                    assert 0 <= x0 - xlo <= x1 - xlo < ncols, (blk, t, ox, (Hi, Wi, fl))
                    assert (y1 - ylo) * ncols + (x1 - xlo) < min(nrows * ncols, FP_SRC)
    return worst


def replay_stores(Ho, Wo, label_offset, twin_offset):
    """The stores of k_logits_ms_merge_tile for one clip, label_u8 / twin_u8 starting at the given byte offsets from a 4-byte
    boundary -> (write counts of the label bytes, of the twin bytes)"""
    plain, twin = np.zeros(Ho * Wo, np.int32), np.zeros(Ho * Wo, np.int32)
    tiles_x = (Wo + FP_W - 1) // FP_W
    for blk in range(((Ho + FP_H - 1) // FP_H) * tiles_x):
        ty, tx = divmod(blk, tiles_x)
        oy0, ox0 = ty * FP_H, tx * FP_W
        for t in range(128):
            oy, oxb = oy0 + (t >> 3), ox0 + (t & 7) * 4
            if oy >= Ho or oxb >= Wo:
                continue
            n = min(4, Wo - oxb)
            dp = oy * Wo + oxb
            dt = oy * Wo + (Wo - 1 - oxb)
            if n == 4 and (label_offset + dp) % 4 == 0:
                plain[dp:dp + 4] += 1                                    # one packed store
            else:
                for k in range(n):
                    plain[dp + k] += 1
            assert dt - (n - 1) >= 0
            if n == 4 and (twin_offset + dt - 3) % 4 == 0:
                twin[dt - 3:dt + 1] += 1                                 # one byte-reversed packed store
            else:
                for k in range(n):
                    twin[dt - k] += 1
    return plain, twin


SIZES = [((41, 49), (53, 65), (160, 192)), ((30, 37), (41, 49), (117, 149))]


@pytest.mark.parametrize('align', [True, False])
@pytest.mark.parametrize('flips', [(False, False), (True, True), (False, True), (True, False)])
@pytest.mark.parametrize('sizes', SIZES)
def test_tile_route_taps_stay_inside_the_stage(sizes, flips, align):
    (h0, w0), (h1, w1), (Ho, Wo) = sizes
    assert Ho >= 2 * max(h0, h1) and Wo >= 2 * max(w0, w1)              # the tile route's precondition
    worst = replay_taps([(h0, w0, flips[0]), (h1, w1, flips[1])], Ho, Wo, align)
    assert worst <= FP_SRC, worst


@pytest.mark.parametrize('sizes', SIZES)
def test_tile_route_writes_every_label_byte_once(sizes):
    Ho, Wo = sizes[2]
    for off in range(4):                                                # label buffers at every byte offset of a word
        plain, twin = replay_stores(Ho, Wo, off, off + Ho * Wo)
        assert (plain == 1).all() and (twin == 1).all()
