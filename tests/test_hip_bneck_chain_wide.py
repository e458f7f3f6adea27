"""rmem_bneck_chain with a 512-channel y (csrc/bottleneck.hip, two column chunks of 256): layer 2's conv3 + shortcut chained into the next
block's conv1, bit for bit against the launches it replaces (the encoder's launch list with the four layer-2 links chained against
the list with separate launches: tests/test_hip_encoder_routes.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.0           # no output of a ReLU
GUARD = 4096              # elements behind the M rows of y and a2
K1, COUT, CIN2 = 128, 512, 256
GEOMS = [(2, 5, 7),       # M = 70: one full row tile plus six rows; the dual form samples a 9 x 13 x 256 map at stride 2
         (1, 2, 3)]       # M = 6: less than one tile; the dual form samples a 4 x 6 x 256 map (the last row and column are skipped)


def seeded(seed, shape, scale=1.0):
    rng = np.random.Generator(np.random.PCG64([seed, 0xC4A1]))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B,Ho,Wo', GEOMS)
@pytest.mark.parametrize('dual', [False, True])
@pytest.mark.parametrize('N2', [128, 256])
def test_wide_chain_is_bit_identical_to_separate_launches(dev, N2, dual, B, Ho, Wo, dt):
    """y [M, 512] and a2 [M, N2] of the chained launch equal rmem_conv2d_nhwc with a residual (dual: rmem_conv1x1_dual_nhwc over
    [b | a 256-channel map sampled at stride 2]) followed by rmem_conv2d_nhwc, element for element; nothing is written behind row M."""
    from rmem_ocu_amd import ops
    M = B * Ho * Wo
    d = lambda t: t.to(dt).to(dev).contiguous()       # noqa: E731
    b = d(seeded(1, (M, K1)))
    kt = K1 + (CIN2 if dual else 0)
    w3, b3 = d(seeded(2, (COUT, kt), 1.0 / kt ** 0.5)), seeded(3, (COUT,), 0.1).to(dev)
    w1, b1 = d(seeded(4, (N2, COUT), 1.0 / COUT ** 0.5)), seeded(5, (N2,), 0.1).to(dev)
    y0, a0 = torch.zeros(M, COUT, dtype=dt, device=dev), torch.zeros(M, N2, dtype=dt, device=dev)
    y1 = torch.full((M * COUT + GUARD,), SENTINEL, dtype=dt, device=dev)
    a1 = torch.full((M * N2 + GUARD,), SENTINEL, dtype=dt, device=dev)
    if dual:
        H2, W2 = (9, 13) if M == 70 else (4, 6)
        x2 = d(seeded(6, (B, H2, W2, CIN2)))
        ops.run(ops.conv1x1_dual(b, x2, w3, b3, y0, H=Ho, W=Wo, Cin=K1, Cout=COUT, H2=H2, W2=W2, Cin2=CIN2, stride2=2, relu=True, batch=B))
        kw = dict(x2=x2, H2=H2, W2=W2, Cin2=CIN2, stride2=2)
    else:
        res = d(seeded(7, (M, COUT)))
        ops.run(ops.conv2d(b, w3, b3, y0, H=Ho, W=Wo, Cin=K1, Cout=COUT, residual=res, relu=True, batch=B))
        kw = dict(residual=res)
    ops.run(ops.conv2d(y0, w1, b1, a0, H=Ho, W=Wo, Cin=COUT, Cout=N2, relu=True, batch=B))
    ops.run(ops.bneck_chain(b, w3, b3, y1, w1, b1, a1, H=Ho, W=Wo, K1=K1, N2=N2, batch=B, Cout=COUT, **kw))
    torch.cuda.synchronize()
    assert y0.float().abs().max().item() > 0.5 and a0.float().abs().max().item() > 0.1      # the case is not degenerate
    assert (y1[M * COUT:] == SENTINEL).all(), 'y: guard region written'
    assert (a1[M * N2:] == SENTINEL).all(), 'a2: guard region written'
    yc, ac = y1[:M * COUT].view(M, COUT), a1[:M * N2].view(M, N2)
    print(f'N2 {N2} dual {dual} M {M} {dt}: y differs in {(yc != y0).sum().item()}, a2 in {(ac != a0).sum().item()} elements')
    assert torch.equal(yc, y0), f'y differs in {(yc != y0).sum().item()} of {y0.numel()} elements'
    assert torch.equal(ac, a0), f'a2 differs in {(ac != a0).sum().item()} of {a0.numel()} elements'
