"""rmem_bneck_block64 (csrc/bneck_block.hip): a whole planes = 64 ResNet bottleneck in one launch against the separate launches it
replaces, bit for bit (the encoder's layer-1 launch list built from it against the chained list: tests/test_hip_encoder_routes.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.0           # no output of a ReLU
GUARD = 4096              # elements behind images * H * W rows
SHAPES = [(1, 3, 1),      # narrower and shorter than any tile
          (2, 9, 70),     # two strips, the second 8 wide
          (3, 17, 64),    # two strips, the second 2 wide
          (1, 5, 62),     # exactly one strip
          (2, 31, 54),
          (1, 40, 125)]
FORMS = ['identity', 'identity_tail', 'projection']


def seeded(seed, shape, scale=1.0):
    rng = np.random.Generator(np.random.PCG64([seed, 0xB10C]))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _guarded(rows, cols, dt, dev):
    return torch.full((rows * cols + GUARD,), SENTINEL, dtype=dt, device=dev)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_block_is_bit_identical_to_separate_launches(dev, monkeypatch, B, H, W, form, dt):
    """y (and a_next) of the one-launch bottleneck equal, bit for bit, conv2d 1x1 + ReLU, conv3x3_direct, conv2d with residual (or
    conv1x1_dual) + ReLU and conv2d 1x1 + ReLU as separate launches; with the rows per run forced to 1, 2 and the whole image (seams
    between runs recompute two rows of conv1), and with the default partition.  conv1's biases are strictly positive, so that a halo
    pixel outside the image that went through conv1 (relu(bias) instead of the 3x3's zero padding) would show.  The outputs carry a
    guard region that must stay untouched, and every image of the batched launch equals its single-image launch."""
    from rmem_ocu_amd import ops
    proj, tail = form == 'projection', form == 'identity_tail'
    cin = 64 if proj else 256
    M = B * H * W
    d = lambda t: t.to(dt).to(dev).contiguous()       # noqa: E731
    x = d(seeded(1, (M, cin)))
    w1, b1 = d(seeded(2, (64, cin), 1.0 / cin ** 0.5)), (seeded(3, (64,), 0.1).abs() + 0.05).to(dev)
    w2, b2 = d(seeded(4, (64, 3, 3, 64), 1.0 / 24)), seeded(5, (64,), 0.1).to(dev)
    w3, b3 = d(seeded(6, (256, 128 if proj else 64), 1.0 / 8)), seeded(7, (256,), 0.1).to(dev)
    w1n, b1n = d(seeded(8, (128, 256), 1.0 / 16)), seeded(9, (128,), 0.1).to(dev)
    assert (b1 > 0).all()

    # the reference: separate launches, computed once
    a, b, y_ref, an_ref = (torch.zeros(M, c, dtype=dt, device=dev) for c in (64, 64, 256, 128))
    ops.run(ops.conv2d(x, w1, b1, a, H=H, W=W, Cin=cin, Cout=64, relu=True, batch=B))
    ops.run(ops.conv3x3_direct(a, w2, b2, b, H=H, W=W, C=64, images=B, relu=True))
    if proj:
        ops.run(ops.conv1x1_dual(b, x, w3, b3, y_ref, H=H, W=W, Cin=64, Cout=256, H2=H, W2=W, Cin2=64, stride2=1, relu=True, batch=B))
    else:
        ops.run(ops.conv2d(b, w3, b3, y_ref, H=H, W=W, Cin=64, Cout=256, residual=x, relu=True, batch=B))
    if tail:
        ops.run(ops.conv2d(y_ref, w1n, b1n, an_ref, H=H, W=W, Cin=256, Cout=128, relu=True, batch=B))
    torch.cuda.synchronize()
    assert y_ref.float().abs().max().item() > 0.5      # the case is not degenerate

    def fused(xs, images):
        m = images * H * W
        y = _guarded(m, 256, dt, dev)
        an = _guarded(m, 128, dt, dev) if tail else None
        kw = dict(w1n=w1n, bias1n=b1n, a_next=an) if tail else {}
        ops.run(ops.bneck_block64(xs, w1, b1, w2, b2, w3, b3, y, H=H, W=W, Cin=cin, images=images, **kw))
        torch.cuda.synchronize()
        assert (y[m * 256:] == SENTINEL).all(), 'y: guard region written'
        assert an is None or (an[m * 128:] == SENTINEL).all(), 'a_next: guard region written'
        return y[:m * 256].view(m, 256), (an[:m * 128].view(m, 128) if tail else None)

    y_def = None
    for rows in (1, 2, 1 << 20, None):
        if rows is None:
            monkeypatch.delenv('RMEM_BNECK_ROWS', raising=False)
        else:
            monkeypatch.setenv('RMEM_BNECK_ROWS', str(rows))
        y, an = fused(x, B)
        ndiff = (y != y_ref).sum().item()
        print(f'{form} {dt} {(B, H, W)} rows per run {rows}: y differs in {ndiff} elements')
        assert torch.equal(y, y_ref), f'rows per run {rows}: y differs in {ndiff} of {y.numel()} elements'
        if tail:
            assert torch.equal(an, an_ref), f'rows per run {rows}: a_next differs in {(an != an_ref).sum().item()} elements'
        y_def = (y, an)
    for i in range(B):
        hw = H * W
        yi, ani = fused(x[i * hw:(i + 1) * hw], 1)
        assert torch.equal(yi, y_def[0][i * hw:(i + 1) * hw]), f'image {i} of the batch differs from its single-image launch'
        if tail:
            assert torch.equal(ani, y_def[1][i * hw:(i + 1) * hw]), f'a_next of image {i} differs from its single-image launch'
