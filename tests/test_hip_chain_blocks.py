"""Block height of the LSTT row chains (csrc/rowchain.hip): a workgroup owns 32 or 64 rows of a clip, and which it is must not
show in any result -- per row the arithmetic is the unfused launch list's, operation for operation, and the GroupNorm partial
sums stay per 32-row block in the 32-row kernel's order."""
import os
from contextlib import contextmanager

import pytest
import torch

from lstt_ref import fill_lstt_state


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_packed = {}


def packed(dt):
    """The synthetic model's packed weights, once per element type."""
    if dt not in _packed:
        from rmem_ocu_amd import build_vos_model, get_config
        from rmem_ocu_amd.weights import synth_state_dict
        cfg = get_config('pre_vost', 'test', 'r50_aotl')
        cfg.MODEL_DTYPE = dt
        model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
        model.load_state_dict(synth_state_dict(0))
        _packed[dt] = model.packed()
    return _packed[dt]


def run_lstt(dev, dt, hw, *, chain=True, stats=False, slots=None, fold=True):
    """Three clips, T = 2, through all three LSTT blocks from the seeded state of test_lstt_chains_are_bit_identical."""
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.group_runtime import GroupRuntime
    B, T = 3, 2
    rt = GroupRuntime(packed(dt), hw, 4, dev, B, lookahead=1)
    rt.chain = chain
    rt.chain_stats = stats
    rt.merge_fold = fold
    L = rt.L
    fill_lstt_state(rt)
    rt.slots = slots if slots is not None else [[1, 3] for _ in range(B)]
    s = torch.cuda.current_stream().cuda_stream
    rt.prepare_pos(s)
    rt.upload_chunks(s)
    prog = rt.prog_lstt(False, T, True)
    ops.run(prog, s)
    torch.cuda.synchronize()
    out = {'x': rt.x, 'dec_in': rt.dec_in[:, 256:], 'qkv': rt.qkv, 'h1': rt.h1, 'h3': rt.h3, 'k4': rt.k4, 'v4': rt.v4,
           'mass': rt.mass[: B * L * T], 'ffn_stats': rt.ffn_stats, **{f'cq{i}': rt.curr_Q[i] for i in range(3)},
           **{f'cv{i}': rt.curr_V[i] for i in range(3)}, **{f'tgt3_{i}': rt.tgt3[i] for i in range(3)}}
    return L, prog, {k: v.clone() for k, v in out.items()}


def assert_same(a, b, keys):
    for k in keys:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (f'{k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} elements differ, '
                                         f'max |d| {(a[k].float() - b[k].float()).abs().max().item():.3e}')


ALL = ('x', 'dec_in', 'qkv', 'h1', 'h3', 'k4', 'v4', 'mass', 'cq0', 'cq1', 'cq2', 'cv0', 'cv1', 'cv2', 'tgt3_0', 'tgt3_1', 'tgt3_2')
_unfused = {}


def unfused(dev, dt, hw):
    """The unfused launch list's results, once per (element type, size)."""
    if (dt, hw) not in _unfused:
        L, prog, out = run_lstt(dev, dt, hw, chain=False)
        assert len(prog) == 48 and not any(op.name.startswith('rmem_lstt_chain') for op in prog)
        _unfused[dt, hw] = (L, out)
    return _unfused[dt, hw]


# network size -> tokens per clip: every remainder class of a 64-row block
SIZES = {(49, 65): 20, (113, 113): 64, (113, 193): 104, (161, 193): 143, (129, 257): 153}


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('hw', sorted(SIZES))
def test_64_row_chains_are_bit_identical_to_the_unfused_list(dev, dt, hw):
    """RMEM_CHAIN_ROWS=64: the chained LSTT against the unfused launch list, bit for bit, at token counts that leave a 64-row
    block's last workgroup with < 32 rows (20), none (64), 40, 15 and 25 rows."""
    Lu, ref = unfused(dev, dt, hw)
    assert Lu == SIZES[hw]
    with env(RMEM_CHAIN_ROWS=64):
        L, prog, got = run_lstt(dev, dt, hw)
    assert L == Lu and len(prog) == 19 and sum(op.name.startswith('rmem_lstt_chain') for op in prog) == 10
    assert_same(ref, got, ALL)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('hw', [(113, 193), (161, 193), (129, 257)])
def test_64_row_chains_write_the_32_row_groupnorm_partial_sums(dev, dt, hw):
    """With the GroupNorm statistics out of linear1's epilogue, 64-row blocks against 32-row blocks: the partial sums (one entry
    per 32-row block, added in the 32-row kernel's order) and everything behind them are bit-identical."""
    outs = []
    for rows in (32, 64):
        with env(RMEM_CHAIN_ROWS=rows):
            L, prog, got = run_lstt(dev, dt, hw, stats=True)
        assert sum(op.name == 'rmem_gn_act_dwconv5x5_prestats_nhwc' for op in prog) == 3
        outs.append(got)
    assert outs[0]['ffn_stats'].abs().max() > 0
    # entries of 32-row blocks a clip does not have stay zero, whatever the block height
    st = outs[1]['ffn_stats'].view(3, 32, 64, 2)
    assert (st[:, :, (SIZES[hw] + 31) // 32:] == 0).all()
    assert_same(outs[0], outs[1], ('ffn_stats', 'h3', 'x', 'dec_in') + ALL)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('rows', [32, 64])
@pytest.mark.parametrize('wgs', ['1', '100', '1000000'])
def test_folded_merge_equals_the_merge_pass(dev, dt, rows, wgs):
    """The memory read's key groups merged by chain B while it stages its rows (the deferred-merge launch) against the merge pass
    + plain chain B, bit for bit: RMEM_ATTN_WGS forcing one group (nothing is deferred), 3 groups of the 8 table rows, and
    one row per group; 143 tokens per clip, so the last block merges rows it does not own."""
    outs = []
    for fold in (False, True):
        with env(RMEM_ATTN_WGS=wgs, RMEM_CHAIN_ROWS=rows):
            L, prog, got = run_lstt(dev, dt, (161, 193), stats=True, fold=fold)
        assert len(prog) == 19 and sum(op.name.startswith('rmem_lstt_chain') for op in prog) == 10
        outs.append(got)
    assert_same(outs[0], outs[1], ALL + ('ffn_stats',))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
@pytest.mark.parametrize('rows', [32, 64])
def test_folded_merge_with_unequal_banks(dev, dt, rows):
    """Clips with banks of 2, 1 and 2 frames in one group: the shorter bank's padded table rows give key groups with l = 0,
    which the folded merge must skip as the merge pass does (one row per group, so such groups exist)."""
    outs = []
    for fold in (False, True):
        with env(RMEM_ATTN_WGS='1000000', RMEM_CHAIN_ROWS=rows):
            L, prog, got = run_lstt(dev, dt, (161, 193), stats=True, fold=fold, slots=[[1, 3], [2], [1, 3]])
        outs.append(got)
    assert_same(outs[0], outs[1], ALL + ('ffn_stats',))


def test_block_height_rule_needs_no_gpu():
    """64 rows when the 32-row grid would not fit one round of the device's compute units, else 32."""
    from rmem_ocu_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    cus = 256      # MI355X
    for L in (1674, 2442, 3600):
        assert ops.lstt_chain_rows(L, 8, cus) == 64
    assert ops.lstt_chain_rows(1674, 4, cus) == 32      # 53 * 4 = 212 workgroups: one round
    for L in SIZES.values():
        assert ops.lstt_chain_rows(L, 3, cus) == 32
    assert ops.lstt_chain_rows(256 * 32, 1, cus) == 32 and ops.lstt_chain_rows(256 * 32 + 1, 1, cus) == 64
