"""Host side of flip testing inside clip groups: the ABI number, and the refusals that need no GPU."""
import os
import re

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_abi_version_is_15_on_both_sides(lib):
    from rmem_ocu_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rmem.h')).read()
    assert re.search(r'#define\s+RMEM_ABI_VERSION\s+15\b', header)
    assert _lib.ABI_VERSION == 15 and lib.rmem_abi_version() == 15
    assert 'rmem_logits_post_flip_pairs' in _lib.SIGNATURES and hasattr(lib, 'rmem_logits_post_flip_pairs')


def test_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    """Refused on the host before anything is launched (the pointers are never dereferenced)."""
    def call(logits, rows, nc, keep, label):
        return lib.rmem_logits_post_flip_pairs(logits, rows, nc, keep, 9, 11, 33, 43, 1, label, None)
    assert call(4096, 3, 11, 6, 4096) != 0 and b'even' in lib.rmem_last_error_string()
    assert call(4096, 4, 17, 6, 4096) != 0 and b'classes' in lib.rmem_last_error_string()
    assert call(4096, 4, 11, 11, 4096) != 0 and b'keep_max_id' in lib.rmem_last_error_string()
    assert call(None, 4, 11, 6, 4096) != 0 and b'null' in lib.rmem_last_error_string()
    assert call(4096, 4, 11, 6, None) != 0 and b'null' in lib.rmem_last_error_string()


def test_op_refuses_an_odd_row_count_before_touching_the_device():
    from rmem_ocu_amd import ops
    from rmem_ocu_amd._lib import RmemError
    lg = torch.zeros(3, 9 * 11, 16)
    lab = torch.zeros(3, 33, 43, dtype=torch.uint8)
    with pytest.raises(RmemError, match='even'):
        ops.logits_post_flip_pairs(lg, nc=11, keep=6, Hi=9, Wi=11, Ho=33, Wo=43, label_u8=lab, rows=3)
    with pytest.raises(RmemError, match='keep'):
        ops.logits_post_flip_pairs(lg, nc=11, keep=11, Hi=9, Wi=11, Ho=33, Wo=43, label_u8=lab, rows=2)
    with pytest.raises(RmemError, match='device tensors'):          # and, as every op, no CPU fallback
        ops.logits_post_flip_pairs(lg, nc=11, keep=6, Hi=9, Wi=11, Ho=33, Wo=43, label_u8=lab, rows=2)


def test_group_engine_refuses_an_odd_row_count_before_touching_the_device():
    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    model = build_vos_model('aot', get_config())
    for clips in (3, 1):
        with pytest.raises(ValueError, match='flip_tta'):
            GroupEngine(model, clips, flip_tta=True)
