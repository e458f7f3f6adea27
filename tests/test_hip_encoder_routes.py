"""BatchEncoder's routes (encoder_batch.EncoderRoutes) at encoder level, 2 images of 97 x 129 (every layer has a ragged last tile:
M = 1650, 442 and 126 rows): the launch list of every route by name and count, x4, x8 and x16 of the routes that replace launches
by bit-identical ones against the default route, and the two routes that are not bit-identical (another summation order in the
row-run stem; split-K plans that follow the GEMM's row count under a split front) run, finite and non-zero."""
import numpy as np
import pytest
import torch

from rmem_ocu_amd.encoder_batch import EncoderRoutes as R

pytestmark = pytest.mark.gpu

COUNTED = ('rmem_bneck_block64', 'rmem_bneck_chain', 'rmem_conv3x3_direct', 'rmem_conv1x1_dual_nhwc', 'rmem_conv2d_nhwc')
DEFAULT = (30, 3, 4, 0, 1, 20)              # launches, then the counts of COUNTED
# routes whose outputs equal the default route's bit for bit (DESIGN.md section 4 and the op-level tests of the launches they swap)
IDENTICAL = {
    'block1_off': (R(block1=False), (34, 0, 7, 3, 1, 21)),
    'chain2_off': (R(chain=(1,)), (34, 3, 0, 0, 2, 27)),
    'chains_off': (R(block1=False, chain=()), (41, 0, 0, 3, 3, 33)),
    'block1_off_direct3_off': (R(block1=False, direct3=()), (34, 0, 7, 0, 1, 24)),
    'direct3_128': (R(direct3=(64, 128)), (30, 3, 4, 3, 1, 17)),
    'stem_direct': (R(stem='direct'), (31, 3, 4, 0, 1, 20)),
}
CLOSE = {
    'stem_rowrun': (R(stem='rowrun'), (31, 3, 4, 0, 1, 21)),
    'front_split_2': (R(front_split=2), (35, 6, 4, 0, 1, 20)),
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _run(P, routes, img, dev):
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.encoder_batch import BatchEncoder
    enc = BatchEncoder(P, (97, 129), 2, dev, routes=routes)
    enc.img_in.copy_(img)
    prog = enc.prog()
    ops.run(prog)
    torch.cuda.synchronize()
    return [o.name for o in prog], [t.clone() for t in enc.enc_out]


@pytest.fixture(scope='module')
def default_route(dev):
    """Per element type: the pack, the two frames, and the launch names and outputs of the default route (computed once)."""
    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.weights import synth_state_dict
    rng = np.random.Generator(np.random.PCG64([20, 0xB10C]))
    img = torch.from_numpy(rng.standard_normal((2, 3, 97, 129)).astype(np.float32)).to(dev)
    made = {}

    def get(dtype):
        if dtype not in made:
            cfg = get_config('pre_vost', 'test', 'r50_aotl')
            cfg.MODEL_DTYPE = dtype
            model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
            model.load_state_dict(synth_state_dict(0, model='aot'))
            P = model.packed()
            names, outs = _run(P, R(), img, dev)
            assert _counts(names) == DEFAULT
            for t in outs:
                assert t.float().abs().max().item() > 0
            made[dtype] = (P, img, names, outs)
        return made[dtype]
    return get


def _counts(names):
    return (len(names),) + tuple(names.count(n) for n in COUNTED)


@pytest.mark.parametrize('route', list(IDENTICAL))
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_route_equals_default_bit_for_bit(dev, default_route, dtype, route):
    """x4, x8 and x16 of the route equal those of the default launch list (layer 1 as three one-launch bottlenecks, the last with the
    tail into layer 2's conv1; links 2.0 -> 2.1 ... 2.3 -> 3.0 chained) bit for bit, and its list has the launches the route names:
    with block1 off no rmem_bneck_block64 and 4 launches more (3 launches were 7), with the layer-2 chain off 4 rmem_bneck_chain
    fewer and 4 launches more."""
    routes, want = IDENTICAL[route]
    P, img, names0, outs0 = default_route(dtype)
    names, outs = _run(P, routes, img, dev)
    assert _counts(names) == want
    if route == 'block1_off':
        assert 'rmem_bneck_block64' not in names and names0.count('rmem_bneck_block64') == 3
        assert len(names) - len(names0) == 4          # 7 launches became 3
    if route == 'chain2_off':
        assert names0.count('rmem_bneck_chain') - names.count('rmem_bneck_chain') == 4
        assert len(names) - len(names0) == 4
    for name, t0, t1 in zip(('x4', 'x8', 'x16'), outs0, outs):
        assert t1.float().abs().max().item() > 0
        assert torch.equal(t0, t1), f'{name} differs in {(t0 != t1).sum().item()} elements'


@pytest.mark.parametrize('route', list(CLOSE))
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_route_runs(dev, default_route, dtype, route):
    """The row-run stem and the split front are not bit-identical to the default (see the module's head): their launch lists by name
    and count, and outputs that are finite and non-zero."""
    routes, want = CLOSE[route]
    P, img, _, _ = default_route(dtype)
    names, outs = _run(P, routes, img, dev)
    assert _counts(names) == want
    if route == 'stem_rowrun':
        assert names[:3] == ['rmem_image_ptrs_to_nhwc8', 'rmem_conv2d_nhwc', 'rmem_maxpool3x3s2_nhwc']
    else:
        assert names.count('rmem_stem7x7s2_pool') == 2 and names.count('rmem_image_ptrs_to_nhwc4p') == 2
    for name, t in zip(('x4', 'x8', 'x16'), outs):
        assert torch.isfinite(t.float()).all(), f'{name} is not finite'
        assert t.float().abs().max().item() > 0, f'{name} is zero'
