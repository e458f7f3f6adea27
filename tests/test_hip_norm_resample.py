"""The primitive normalisation / activation kernels (rmem_ocu_amd/csrc/norm_act.hip) and the plain resampling kernels
(rmem_ocu_amd/csrc/resample.hip) against the float64 references of tests/norm_ref.py, per element:
|got - ref| <= ulp(ref) + c_op * 2^-24 * cond_op (exact operations: torch.equal), on the adversarial cases of that module, in both
element types.  Every output buffer is pre-filled with a sentinel and is wider / longer than what the launch may write; what lies
outside must still hold the sentinel.  Each test prints the worst err / bound it saw."""
import pytest
import torch

import norm_ref as R
from norm_ref import DTS, EPS, F32, SENTINEL
from test_hip_ops import seeded

pytestmark = pytest.mark.gpu
dts = pytest.mark.parametrize('dt', DTS, ids=['bf16', 'f16'])


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def up(t, dev, dt=None):
    """fp32 values -> device tensor (of the 16-bit type dt: the values were rounded through it, so this is exact)."""
    return None if t is None else (t if dt is None else t.to(dt)).contiguous().to(dev)


def guard(shape, dt, dev):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENTINEL, dtype=dt, device=dev)


def untouched(t):
    return bool((t == SENTINEL).all())


class Worst:
    """Collects err / bound over the checks of one test and prints the worst on exit (fp32 outputs, whose bound has no ulp term,
    also on their own: the 16-bit ones sit at the half unit of a correct rounding)."""

    def __init__(self, what):
        self.what, self.ratio, self.at, self.f32 = what, 0.0, '', None

    def check(self, label, got, ref, bnd):
        r = R.worst(got, ref, bnd)
        if r > self.ratio:
            self.ratio, self.at = r, label
        if got.dtype == F32:
            self.f32 = max(self.f32 or 0.0, r)
        assert r <= 1, f'{self.what} {label}: err / bound = {r:.4g}'

    def done(self):
        print(f'{self.what}: worst err / bound = {self.ratio:.3g} ({self.at})' + ('' if self.f32 is None else f'; fp32 outputs {self.f32:.3g}'))


# ------------------------------------------------------------------ LayerNorm
@dts
@pytest.mark.parametrize('case', R.LN256_CASES, ids=lambda c: f'M{c.M}-a{"f32" if c.a_f32 else "16"}-b{c.b}')
def test_layernorm256(dev, case, dt):
    """Strided operands (a: columns 256..511 of a 768-wide fused row; b in a 512-wide row), y at column 256 of a 1024-wide row, ypos
    in a 512-wide row, yf in 260-wide rows; all three outputs at once, then each alone (bit-identical to the joint launch)."""
    from rmem_ocu_amd import ops
    M, L = case.M, R.LN256_LD
    x = R.ln256_inputs(case, dt)
    a = torch.zeros(M, L['lda'])
    a[:, 256:512] = x['a']
    b = None
    if x['b'] is not None:
        b = torch.zeros(M, L['ldb'])
        b[:, :256] = x['b']
    ad, bd = up(a, dev, None if case.a_f32 else dt), up(b, dev, None if case.b == 'f32' else dt)
    g, be, pos = up(x['gamma'], dev), up(x['beta'], dev), up(x['pos'], dev)
    args = (x['a'], x['b'], x['gamma'], x['beta'], EPS, x['pos'])
    (ln, lnp), (c, cp) = R.layernorm_ref(*args), R.layernorm_cond(*args)
    w = Worst(f'layernorm256 {case} {dt}')
    outs = {}
    for which in ('all', 'y', 'ypos', 'yf'):
        y, yp, yf = guard((M + 1, L['ldy']), dt, dev), guard((M + 1, L['ldyp']), dt, dev), guard((M + 1, L['ldyf']), F32, dev)
        ops.run(ops.layernorm256(ad.view(-1)[256:], g, be, M=M, lda=L['lda'], b=bd, ldb=L['ldb'],
                                 y=y.view(-1)[L['ycol']:] if which in ('all', 'y') else None, ldy=L['ldy'],
                                 pos=pos if which in ('all', 'ypos') else None, ypos=yp if which in ('all', 'ypos') else None, ldyp=L['ldyp'],
                                 yf=yf if which in ('all', 'yf') else None, ldyf=L['ldyf']))
        torch.cuda.synchronize()
        assert untouched(y[M:]) and untouched(y[:, :256]) and untouched(y[:, 512:]) and untouched(yp[M:]) and untouched(yp[:, 256:])
        assert untouched(yf[M:]) and untouched(yf[:, 256:])
        if which == 'all':
            outs = dict(y=y, ypos=yp, yf=yf)
            w.check('yf', yf[:M, :256], ln, R.bound(ln, c, R.C_LN))
            w.check('y', y[:M, 256:512], ln, R.bound(ln, c, R.C_LN, dt))
            w.check('ypos', yp[:M, :256], lnp, R.bound(lnp, cp, R.C_LN, dt))
        else:
            for k, t in dict(y=y, ypos=yp, yf=yf).items():
                assert torch.equal(t, outs[k]) if k == which else untouched(t), (which, k)
    w.done()


@dts
@pytest.mark.parametrize('C', R.LN_GENERIC_C)
def test_layernorm_generic(dev, C, dt):
    from rmem_ocu_amd import ops
    w = Worst(f'layernorm C={C} {dt}')
    for M in R.LN_GENERIC_M:
        for a_f32 in (True, False):
            x = R.ln_generic_inputs(C, M, dt, a_f32)
            a = torch.zeros(M, C + 8)
            a[:, :C] = x['a']
            y, yf = guard((M + 1, 2 * C), dt, dev), guard((M + 1, C + 4), F32, dev)
            ops.run(ops.layernorm(up(a, dev, None if a_f32 else dt), up(x['gamma'], dev), up(x['beta'], dev), M=M, C=C, lda=C + 8,
                                  y=y, ldy=2 * C, yf=yf, ldyf=C + 4))
            torch.cuda.synchronize()
            assert untouched(y[M:]) and untouched(y[:, C:]) and untouched(yf[M:]) and untouched(yf[:, C:])
            args = (x['a'], None, x['gamma'], x['beta'])
            ln, c = R.layernorm_ref(*args)[0], R.layernorm_cond(*args)[0]
            w.check(f'yf M={M} f32={a_f32}', yf[:M, :C], ln, R.bound(ln, c, R.C_LN))
            w.check(f'y M={M} f32={a_f32}', y[:M, :C], ln, R.bound(ln, c, R.C_LN, dt))
    w.done()


@dts
@pytest.mark.parametrize('C', R.PATCH_C)
def test_patch_merge_ln(dev, C, dt):
    from rmem_ocu_amd import ops
    w = Worst(f'patch_merge_ln C={C} {dt}')
    for H, W in R.PATCH_HW:
        for images in R.PATCH_IMAGES:
            x = R.patch_inputs(C, H, W, images)
            T = ((H + 1) // 2) * ((W + 1) // 2)
            y = guard((images * T + 1, 4 * C), dt, dev)
            ops.run(ops.patch_merge_ln(up(x['x'], dev), up(x['gamma'], dev), up(x['beta'], dev), y, H=H, W=W, C=C, images=images))
            torch.cuda.synchronize()
            assert untouched(y[images * T:])
            args = (x['x'], x['gamma'], x['beta'])
            ref = R.patch_merge_ref(*args)
            w.check(f'{H}x{W} images={images}', y[:images * T].view(images, T, 4 * C), ref, R.bound(ref, R.patch_merge_cond(*args), R.C_LN, dt))
    w.done()


# ------------------------------------------------------------------ GroupNorm
def run_groupnorm(dev, w, case, dt, in_f32, images, acts):
    from rmem_ocu_amd import ops
    x, g, b = R.gn_inputs(case, dt, in_f32, images)
    xd, gd, bd = up(x, dev, None if in_f32 else dt), up(g, dev), up(b, dev)
    cond = R.groupnorm_cond(x, case.groups, g, b)
    for act in acts:
        y = guard((images * case.M + 1, case.C), dt, dev)
        ws = ops.groupnorm_workspace(case.groups, dev, images).fill_(float('nan'))          # every partial must be written
        ops.run(ops.groupnorm(xd, gd, bd, y, ws, M=case.M, C=case.C, groups=case.groups, act=act, images=images))
        torch.cuda.synchronize()
        assert untouched(y[images * case.M:]) and bool(torch.isfinite(ws).all())
        ref = R.groupnorm_ref(x, case.groups, g, b, EPS, act)
        w.check(f'f32={in_f32} images={images} act={act}', y[:images * case.M].view(images, case.M, case.C), ref, R.bound(ref, cond, R.C_GN, dt))


@dts
@pytest.mark.parametrize('case', R.GN_CASES, ids=lambda c: c.name)
def test_groupnorm(dev, case, dt):
    """Both launch branches, both input types, three images with their own statistics, the three activations."""
    w = Worst(f'groupnorm {case.name} {dt}')
    for in_f32, images in R.GN_VARIANTS:
        run_groupnorm(dev, w, case, dt, in_f32, images, (0, 1, 2))
    w.done()


@dts
@pytest.mark.parametrize('in_f32', [False, True], ids=['in16', 'in32'])
def test_groupnorm_generic_above_grid_cap(dev, in_f32, dt):
    """k_gn_apply's grid-stride loop runs a second, ragged pass."""
    w = Worst(f'groupnorm {R.GN_CAP_CASE.name} {dt}')
    run_groupnorm(dev, w, R.GN_CAP_CASE, dt, in_f32, 1, (1,))
    w.done()


@dts
@pytest.mark.parametrize('case', R.HEAD_CASES, ids=lambda c: f'{c.H}x{c.W}')
def test_groupnorm_head(dev, case, dt):
    from rmem_ocu_amd import ops
    M, C, N = case.H * case.W, case.C, R.HEAD_N
    w = Worst(f'groupnorm_head {case.H}x{case.W} {dt}')
    for images in (1, 3):
        x = R.map_inputs(case, dt, images)
        y = guard((images * M + 1, 16), F32, dev)
        ws = ops.groupnorm_workspace(case.groups, dev, images).fill_(float('nan'))
        ops.run(ops.groupnorm_head(up(x['x'], dev, dt), up(x['gamma'], dev), up(x['beta'], dev), up(x['w'], dev, dt), up(x['bias'], dev), y, ws,
                                   M=M, C=C, groups=case.groups, N=N, ldy=16, act=1, images=images))
        torch.cuda.synchronize()
        assert untouched(y[images * M:]) and untouched(y[:, N:])
        args = (x['x'], case.groups, x['gamma'], x['beta'])
        mid = R.groupnorm_ref(*args, EPS, 1)
        mb = R.bound(mid, R.groupnorm_cond(*args), R.C_GN, dt)
        w.check(f'images={images}', y[:images * M, :N].view(images, M, N), R.head_ref(mid, x['w'], x['bias']), R.head_bound(mid, mb, x['w'], x['bias']))
    w.done()


@dts
@pytest.mark.parametrize('case', R.FUSED_CASES, ids=lambda c: f'{c.H}x{c.W}x{c.C}')
def test_gn_act_dwconv5x5(dev, case, dt):
    from rmem_ocu_amd import ops
    H, W, C, M = case.H, case.W, case.C, case.H * case.W
    w = Worst(f'gn_act_dwconv5x5 {H}x{W}x{C} {dt}')
    for images in (1, 3):
        x = R.map_inputs(case, dt, images)
        y = guard((images * M + 1, C), dt, dev)
        ws = ops.groupnorm_workspace(case.groups, dev, images).fill_(float('nan'))
        ops.run(ops.gn_act_dwconv5x5(up(x['x'], dev, dt), up(x['gamma'], dev), up(x['beta'], dev), up(x['taps'], dev), y, ws, H=H, W=W, C=C,
                                     groups=case.groups, act=2, images=images))
        torch.cuda.synchronize()
        assert untouched(y[images * M:])
        args = (x['x'], case.groups, x['gamma'], x['beta'])
        mid = R.groupnorm_ref(*args, EPS, 2)
        mb = R.bound(mid, R.groupnorm_cond(*args), R.C_GN, dt)
        for i in range(images):
            ref = R.dwconv5x5_ref(mid[i], x['taps'], H, W)
            w.check(f'images={images} image {i}', y[i * M:(i + 1) * M], ref, R.fused_bound(mid[i], mb[i], ref, x['taps'].double(), H, W, dt))
    w.done()


@dts
def test_dwconv5x5(dev, dt):
    from rmem_ocu_amd import ops
    w = Worst(f'dwconv5x5 {dt}')
    for H, W in R.MAPS:
        for C in R.DWCONV_C:
            x, taps = R.dwconv_inputs(H, W, C, dt)
            y = guard((H * W + 1, C), dt, dev)
            ops.run(ops.dwconv5x5(up(x, dev, dt), up(taps, dev), y, H=H, W=W, C=C))
            torch.cuda.synchronize()
            assert untouched(y[H * W:])
            ref = R.dwconv5x5_ref(x, taps, H, W)
            w.check(f'{H}x{W}x{C}', y[:H * W], ref, R.bound(ref, R.dwconv_cond(x, taps, H, W), R.C_DOT, dt))
    w.done()


# ------------------------------------------------------------------ add
def add_operands(seed, n, dt, dev):
    a, b = R.through(seeded(seed, (n,), 3.0), dt), R.through(seeded(seed + 1, (n,), 0.7), dt)
    return up(a, dev, dt), up(b, dev, dt), (a + b).to(dt)


@dts
@pytest.mark.parametrize('n', R.ADD_N)
def test_add16(dev, n, dt):
    """Exact (one rounding of the fp32 sum); beyond the grid cap the loop runs a second pass with a ragged tail; in place (y is a)."""
    from rmem_ocu_amd import ops
    a, b, ref = add_operands(9100, n, dt, dev)
    y = guard(n + 8, dt, dev)
    ops.run(ops.add16(a, b, y, n))
    torch.cuda.synchronize()
    assert torch.equal(y[:n].cpu(), ref) and untouched(y[n:])
    buf = guard(n + 8, dt, dev)
    buf[:n] = a
    ops.run(ops.add16(buf, b, buf, n))
    torch.cuda.synchronize()
    assert torch.equal(buf[:n].cpu(), ref) and untouched(buf[n:])


@dts
@pytest.mark.parametrize('problems,n', R.ADD_GROUPED)
def test_add16_grouped(dev, problems, n, dt):
    from rmem_ocu_amd import ops
    trip = [add_operands(9200 + 2 * i, n, dt, dev) for i in range(problems)]
    ys = [guard(n + 8, dt, dev) for _ in range(problems)]
    ops.run(ops.add16_grouped([t[0] for t in trip], [t[1] for t in trip], ys, n))
    torch.cuda.synchronize()
    for (a, b, ref), y in zip(trip, ys):
        assert torch.equal(y[:n].cpu(), ref) and untouched(y[n:])
    bufs = [guard(n + 8, dt, dev) for _ in range(problems)]
    for (a, b, ref), buf in zip(trip, bufs):
        buf[:n] = a
    ops.run(ops.add16_grouped(bufs, [t[1] for t in trip], bufs, n))          # in place, as group_runtime.py adds the id embedding
    torch.cuda.synchronize()
    for (a, b, ref), buf in zip(trip, bufs):
        assert torch.equal(buf[:n].cpu(), ref) and untouched(buf[n:])


# ------------------------------------------------------------------ resampling
@dts
def test_maxpool3x3s2(dev, dt):
    from rmem_ocu_amd import ops
    for H, W in R.POOL_HW:
        for C in R.POOL_C:
            for images in R.POOL_IMAGES:
                for negative in (False, True) if (H, W) in ((2, 5), (49, 65)) else (False,):
                    x = R.pool_inputs(H, W, C, images, dt, negative)
                    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                    y = guard((images * Ho * Wo + 1, C), dt, dev)
                    ops.run(ops.maxpool3x3s2(up(x, dev, dt), y, H=H, W=W, C=C, images=images))
                    torch.cuda.synchronize()
                    ref = R.maxpool3x3s2_ref(x).reshape(-1, C).to(dt)
                    assert torch.equal(y[:images * Ho * Wo].cpu(), ref) and untouched(y[images * Ho * Wo:]), (H, W, C, images, negative)


@dts
@pytest.mark.parametrize('align', [True, False], ids=['align', 'half-pixel'])
def test_bilinear(dev, align, dt):
    from rmem_ocu_amd import ops
    w = Worst(f'bilinear align={align} {dt}')
    for Hi, Wi, Ho, Wo in R.BILINEAR_GEOMS:
        for C in R.BILINEAR_C:
            images = 2 if C == 8 else 1
            x = R.bilinear_inputs(Hi, Wi, C, dt, images)
            y = guard((images * Ho * Wo + 1, C), dt, dev)
            ops.run(ops.bilinear(up(x, dev, dt), y, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=C, align_corners=align, images=images))
            torch.cuda.synchronize()
            assert untouched(y[images * Ho * Wo:])
            ref = R.bilinear_ref(x, Ho, Wo, align)
            w.check(f'{Hi}x{Wi}->{Ho}x{Wo} C={C}', y[:images * Ho * Wo].view(images, Ho, Wo, C), ref,
                    R.bound(ref, R.bilinear_cond(x, Ho, Wo, align), R.C_BILINEAR, dt))
    w.done()


@dts
def test_image_to_nhwc8_both_forms(dev, dt):
    from rmem_ocu_amd import ops
    for H, W in R.LAYOUT_HW:
        for images in (1, 2):
            img = seeded(9300 + H, (images, 3, H, W), 2.0)
            ref = torch.zeros(images, H * W, 8, dtype=dt)
            ref[:, :, :3] = img.to(dt).permute(0, 2, 3, 1).reshape(images, H * W, 3)
            out = guard((images * H * W + 1, 8), dt, dev)
            ops.run(ops.image_to_nhwc8(up(img, dev), out, H=H, W=W, images=images))
            frames = [up(img[i], dev) for i in reversed(range(images))]                      # separate allocations, in another order
            table = torch.tensor([f.data_ptr() for f in reversed(frames)], dtype=torch.int64, device=dev)
            out2 = guard((images * H * W + 1, 8), dt, dev)
            ops.run(ops.image_ptrs_to_nhwc8(table, out2, H=H, W=W, images=images))
            torch.cuda.synchronize()
            for o in (out, out2):
                assert torch.equal(o[:images * H * W].cpu().view(images, H * W, 8), ref) and untouched(o[images * H * W:]), (H, W, images)


def test_resize_nearest_flip(dev):
    from rmem_ocu_amd import ops
    for Hs, Ws, Hd, Wd in R.NEAREST_GEOMS:
        src = seeded(9400 + Hs, (2, Hs, Ws))
        for flip in (False, True):
            dst = guard((3, Hd, Wd), F32, dev)
            ops.run(ops.resize_nearest_flip(up(src, dev), dst[:2], flip=flip))
            torch.cuda.synchronize()
            assert torch.equal(dst[:2].cpu(), R.nearest_ref(src, Hd, Wd, flip=flip)) and untouched(dst[2:]), (Hs, Ws, Hd, Wd, flip)


@dts
def test_label_to_onehot16(dev, dt):
    """uint8 and fp32 labels, the ignore label 255, ids beyond the class count, two images, resize ratios at which the fp32 index rule
    differs from the exact one (norm_ref.NEAREST_PAIR)."""
    from rmem_ocu_amd import ops
    for Hs, Ws, Hd, Wd in R.NEAREST_GEOMS:
        lab = R.label_inputs(Hs, Ws, 2)
        ref = R.onehot16_ref(lab, Hd, Wd, 11).to(dt)
        for labels in (lab.to(torch.uint8), lab.float()):
            out = guard((2 * Hd * Wd + 1, 16), dt, dev)
            ops.run(ops.label_to_onehot16(labels.to(dev), out, Hs=Hs, Ws=Ws, Hd=Hd, Wd=Wd, ncls=11, images=2))
            torch.cuda.synchronize()
            assert torch.equal(out[:2 * Hd * Wd].cpu().view(2, Hd * Wd, 16), ref) and untouched(out[2 * Hd * Wd:]), (Hs, Ws, Hd, Wd, labels.dtype)


@pytest.mark.parametrize('T', R.EVICT_T)
def test_evict_scores(dev, T):
    from rmem_ocu_amd import ops
    g = R.EVICT_GEOM
    lg, mass = R.evict_inputs(T)
    lgn = torch.zeros(g['Hi'] * g['Wi'], 16)
    lgn[:, :g['nc']] = lg.reshape(-1, g['nc'])
    sc = guard(32 + 64 * 32, F32, dev)
    ops.run(ops.evict_scores(up(lgn, dev), up(mass, dev), sc, ldl=16, nc=g['nc'], keep=g['keep'], Hi=g['Hi'], Wi=g['Wi'], He=g['He'], We=g['We'], T=T))
    torch.cuda.synchronize()
    assert untouched(sc[T:32])
    args = (lg, mass, g['keep'], g['He'], g['We'])
    w = Worst(f'evict_scores T={T}')
    w.check('scores', sc[:T], R.evict_ref(*args), R.bound(R.evict_ref(*args), R.evict_cond(*args), R.C_EVICT))
    w.done()


@pytest.mark.parametrize('block_bytes', R.SCATTER_BLOCKS)
def test_scatter_blocks(dev, block_bytes):
    """Three clips' blocks into permuted slots of a bank whose slots are 16 bytes longer than a block; a negative slot skips its clip."""
    from rmem_ocu_amd import ops
    n, slots_n, slot_bytes, fill = R.SCATTER_CLIPS, 5, block_bytes + 16, 0xA5
    gen = torch.Generator().manual_seed(9500)
    src = torch.randint(0, 256, (n, block_bytes), generator=gen, dtype=torch.uint8)
    for slots in ([4, 0, 2], [-1, 3, 1]):
        dst = torch.full((slots_n, slot_bytes), fill, dtype=torch.uint8, device=dev)
        ops.run(ops.scatter_blocks(src.to(dev), dst, torch.tensor(slots, dtype=torch.int32, device=dev), nclips=n, block_bytes=block_bytes,
                                   slot_bytes=slot_bytes))
        torch.cuda.synchronize()
        ref = torch.full((slots_n, slot_bytes), fill, dtype=torch.uint8)
        for c, s in enumerate(slots):
            if s >= 0:
                ref[s, :block_bytes] = src[c]
        assert torch.equal(dst.cpu(), ref), slots
