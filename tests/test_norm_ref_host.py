"""CPU checks of tests/norm_ref.py, the yardstick of tests/test_hip_norm_resample.py: the float64 references agree with torch's own
operators and the oracle; the fp32 emulation of every kernel formula stays within the per-element bound with the chosen constants,
and the constants are no more than 4x what the emulation needs; every mutation a case exists for moves the reference by more than 5x
the bound somewhere; and the GPU case list reaches the launch branches it was chosen for."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from norm_ref import BF16, DTS, EPS, F16, F32, F64, through
from test_hip_ops import seeded


def rel_err(got, ref):
    return ((got.double() - ref.double()).abs().max() / ref.abs().max()).item()


def nchw(x):          # [images, H, W, C] -> [images, C, H, W]
    return x.permute(0, 3, 1, 2).contiguous()


def gn_case(name):
    return next(c for c in R.GN_CASES if c.name == name)


# ------------------------------------------------------------------ references against an independent statement
def test_layernorm_and_patch_merge_refs_match_torch():
    for case in R.LN256_CASES:
        x = R.ln256_inputs(case, BF16)
        v = x['a'] if x['b'] is None else x['a'] + x['b']
        ln, lnp = R.layernorm_ref(x['a'], x['b'], x['gamma'], x['beta'], EPS, x['pos'])
        # loose: the fp32 operator itself loses |mean| / std * 2^-24 on the mean-30 row
        assert rel_err(F.layer_norm(v, (256,), x['gamma'], x['beta'], EPS), ln) < 1e-4
        assert torch.equal(lnp, ln + x['pos'].double())
    C, H, W = 128, 9, 11
    x = R.patch_inputs(C, H, W, 3)
    xp = F.pad(x['x'], (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1).view(3, -1, 4 * C)   # swin_transformer.py
    assert rel_err(F.layer_norm(cat, (4 * C,), x['gamma'], x['beta'], EPS), R.patch_merge_ref(x['x'], x['gamma'], x['beta'])) < 1e-5


@pytest.mark.parametrize('act', [0, 1, 2])
def test_groupnorm_ref_matches_torch(act):
    case = gn_case('rows-256')
    x, g, b = R.gn_inputs(case, BF16, False, 3)
    t = F.group_norm(x.double().permute(0, 2, 1), case.groups, g.double(), b.double(), EPS).permute(0, 2, 1)
    t = F.relu(t) if act == 1 else F.gelu(t) if act == 2 else t
    assert (t - R.groupnorm_ref(x, case.groups, g, b, EPS, act)).abs().max().item() < 1e-9
    z = R._gn_terms(x, case.groups, g, b, EPS)[2]
    assert z.min().item() < -3 and z.max().item() > 3


def test_gn_gelu_dwconv_ref_matches_oracle():
    from oracle import ref_cpu as O
    h, wd, C = 9, 11, 64
    x = seeded(931, (h * wd, 1, C)) * 2 + 0.5
    w = {'m.gn.weight': 1 + 0.1 * seeded(932, (C,)), 'm.gn.bias': 0.1 * seeded(933, (C,)), 'm.conv.weight': seeded(934, (C, 1, 5, 5), 0.2)}
    mid = R.groupnorm_ref(x[:, 0][None], 32, w['m.gn.weight'], w['m.gn.bias'], EPS, 2)[0]
    ref = R.dwconv5x5_ref(mid, w['m.conv.weight'].view(C, 25).t(), h, wd)
    assert rel_err(O.gn_gelu_dwconv(x, (h, wd), w, 'm')[:, 0], ref) < 1e-5


def test_resample_refs_match_torch():
    x = R.pool_inputs(49, 65, 8, 2, BF16)
    assert torch.equal(F.max_pool2d(nchw(x), 3, 2, 1).double(), nchw(R.maxpool3x3s2_ref(x)))
    x = R.pool_inputs(2, 5, 8, 1, BF16, negative=True)
    assert torch.equal(F.max_pool2d(nchw(x), 3, 2, 1).double(), nchw(R.maxpool3x3s2_ref(x)))
    for Hi, Wi, Ho, Wo in R.BILINEAR_GEOMS:
        for ac in (True, False):
            x = R.bilinear_inputs(Hi, Wi, 8, BF16)
            t = F.interpolate(nchw(x), size=(Ho, Wo), mode='bilinear', align_corners=ac)
            assert (t.double() - nchw(R.bilinear_ref(x, Ho, Wo, ac))).abs().max().item() < 1e-4, (Hi, Wi, Ho, Wo, ac)
    for Hs, Ws, Hd, Wd in R.NEAREST_GEOMS:
        src = seeded(941, (2, Hs, Ws))
        assert torch.equal(F.interpolate(src[None], size=(Hd, Wd), mode='nearest')[0], R.nearest_ref(src, Hd, Wd))
        assert torch.equal(F.interpolate(src.flip(-1)[None], size=(Hd, Wd), mode='nearest')[0], R.nearest_ref(src, Hd, Wd, flip=True))
    lab = R.label_inputs(13, 21, 2)
    oh = R.onehot16_ref(lab, 29, 47, 11)
    near = F.interpolate(lab[:, None].float(), size=(29, 47), mode='nearest')[:, 0].long().view(2, -1)
    assert torch.equal(oh[..., :11].argmax(-1)[near < 11], near[near < 11]) and torch.equal(oh[..., 11] == 1, near == 255)
    assert (oh.sum(-1)[near < 11] == 1).all() and (oh.sum(-1)[(near >= 11) & (near != 255)] == 0).all() and (oh[..., 12:] == 0).all()
    assert (near == 255).any() and (near == 13).any()


def test_evict_ref_matches_torch():
    g = R.EVICT_GEOM
    lg, mass = R.evict_inputs(5)
    m = lg.clone()
    m[..., g['keep'] + 1:] = -1e10
    up = F.interpolate(m.permute(2, 0, 1)[None], size=(g['He'], g['We']), mode='bilinear', align_corners=True)
    fg = 1 - torch.softmax(up, 1)[0, 0].flatten()
    assert rel_err((mass * fg[:, None]).sum(0), R.evict_ref(lg, mass, g['keep'], g['He'], g['We'])) < 1e-5


def test_nearest_pair_is_a_case_where_fp32_floor_differs():
    n_in, n_out = R.NEAREST_PAIR
    assert n_out % n_in and not torch.equal(R.nearest_index(n_in, n_out), R.nearest_index(n_in, n_out, 'f64'))
    assert any((Hs, Hd) == R.NEAREST_PAIR or (Ws, Wd) == R.NEAREST_PAIR for Hs, Ws, Hd, Wd in R.NEAREST_GEOMS)


def test_ulp_is_the_spacing_of_the_element_type():
    v = torch.tensor([0.0, 1.0, 1.5, 1.9999, 2.0, -3.0, 1e-3, 100.5, 6e-8], dtype=F64)
    for dt in DTS:
        up = torch.nextafter(v.abs().to(dt), torch.tensor(math.inf, dtype=dt)).double() if dt is F16 else None
        u = R.ulp(v, dt)
        assert u[1].item() == 2.0 ** -R._MANT[dt] and u[4].item() == 2.0 ** (1 - R._MANT[dt]) and u[3].item() == u[1].item()
        if up is not None:
            exact = v.abs().to(dt).double() == v.abs()
            assert torch.equal((up - v.abs())[exact], u[exact])


# ------------------------------------------------------------------ the emulations: (family, label, emulation, reference, cond, output types)
def ln_items():
    for dt in DTS:
        for case in R.LN256_CASES:
            x = R.ln256_inputs(case, dt)
            args = (x['a'], x['b'], x['gamma'], x['beta'], EPS, x['pos'])
            for e, r, c, what in zip(R.layernorm_emu(*args), R.layernorm_ref(*args), R.layernorm_cond(*args), ('ln', 'ln+pos')):
                yield f'ln256 {case} {what}', e, r, c, (None, dt)
        for C in R.LN_GENERIC_C:
            for M in R.LN_GENERIC_M:
                for f32 in (True, False):
                    x = R.ln_generic_inputs(C, M, dt, f32)
                    args = (x['a'], None, x['gamma'], x['beta'])
                    yield f'ln{C} M={M} f32={f32}', R.layernorm_emu(*args)[0], R.layernorm_ref(*args)[0], R.layernorm_cond(*args)[0], (None, dt)
    for C in R.PATCH_C:
        for H, W in R.PATCH_HW:
            x = R.patch_inputs(C, H, W, 3)
            args = (x['x'], x['gamma'], x['beta'])
            yield f'patch {C} {H}x{W}', R.patch_merge_emu(*args), R.patch_merge_ref(*args), R.patch_merge_cond(*args), DTS


def gn_items():
    for dt in DTS:
        for case in R.GN_CASES + (R.GN_CAP_CASE,):
            cap = case is R.GN_CAP_CASE
            for f32, images in ((False, 1), (True, 1)) if cap else R.GN_VARIANTS:
                x, g, b = R.gn_inputs(case, dt, f32, images)
                cond = R.groupnorm_cond(x, case.groups, g, b)
                for act in (1,) if cap else (0, 1, 2):
                    yield (f'gn {case.name} {dt} f32={f32} images={images} act={act}', R.groupnorm_emu(x, case.groups, g, b, EPS, act),
                           R.groupnorm_ref(x, case.groups, g, b, EPS, act), cond, (dt,))


def dot_items():
    for dt in DTS:
        for H, W in R.MAPS:
            for C in R.DWCONV_C:
                x, w = R.dwconv_inputs(H, W, C, dt)
                yield f'dwconv {H}x{W}x{C}', R.dwconv_emu(x, w, H, W), R.dwconv5x5_ref(x, w, H, W), R.dwconv_cond(x, w, H, W), (dt,)
        for case in R.HEAD_CASES:
            x = R.map_inputs(case, dt)
            mid = through(R.groupnorm_ref(x['x'], case.groups, x['gamma'], x['beta'], EPS, 1)[0].float(), dt)
            yield (f'head product {case.H}x{case.W}', mid @ x['w'].t() + x['bias'], R.head_ref(mid.double(), x['w'], x['bias']),
                   mid.double().abs() @ x['w'].double().abs().t() + x['bias'].double().abs(), (None,))


def bilinear_items():
    for dt in DTS:
        for Hi, Wi, Ho, Wo in R.BILINEAR_GEOMS:
            for C in R.BILINEAR_C:
                for ac in (True, False):
                    x = R.bilinear_inputs(Hi, Wi, C, dt)
                    yield (f'bilinear {Hi}x{Wi}->{Ho}x{Wo} C={C} ac={ac}', R.bilinear_ref(x, Ho, Wo, ac, dtype=F32), R.bilinear_ref(x, Ho, Wo, ac),
                           R.bilinear_cond(x, Ho, Wo, ac), (dt,))


def evict_items():
    g = R.EVICT_GEOM
    for T in R.EVICT_T:
        lg, mass = R.evict_inputs(T)
        args = (lg, mass, g['keep'], g['He'], g['We'])
        yield f'evict T={T}', R.evict_emu(*args), R.evict_ref(*args), R.evict_cond(*args), (None,)


FAMILIES = {'LN': ln_items, 'GN': gn_items, 'DOT': dot_items, 'BILINEAR': bilinear_items, 'EVICT': evict_items}


@pytest.mark.parametrize('family', list(FAMILIES))
def test_emulation_within_bound_and_constant_not_loose(family):
    """The reference alone fits the bound (the fp32 formula, in the kernel's reduction structure, is inside it with the chosen
    constant), and the constant is what norm_ref.py says it is: 4x the measured need, rounded up to a power of two."""
    measured, chosen = getattr(R, 'MEASURED_C_' + family), getattr(R, 'C_' + family)
    need, at, ratio = 0.0, None, 0.0
    for label, emu, ref, cond, dts in FAMILIES[family]():
        for dt in dts:
            got = emu if dt is None else through(emu, dt)
            c = R.needed_c(got, ref, cond, dt)
            if c > need:
                need, at = c, (label, dt)
            ratio = max(ratio, R.worst(got, ref, R.bound(ref, cond, chosen, dt)))
    print(f'{family}: emulation needs c = {need:.4g} at {at}; recorded {measured}, chosen {chosen}; worst err / bound {ratio:.3g}')
    assert ratio <= 1
    assert need <= measured, f'{family}: a case needs c = {need:.4g}, above the recorded measurement {measured}'
    assert measured <= 1.25 * need + 1e-9, f'{family}: the recorded measurement {measured} is stale (the cases need {need:.4g})'
    assert chosen == R.c_from(measured) and chosen <= max(1.0, R.pow2_ceil(4 * measured))


def test_fused_products_emulation_within_bound():
    """act(GroupNorm) stored in the element type, then the head's product / the depth-wise taps, in fp32: inside head_bound / fused_bound."""
    for dt in DTS:
        for case in R.HEAD_CASES:
            x = R.map_inputs(case, dt)
            args = (x['x'], case.groups, x['gamma'], x['beta'], EPS, 1)
            mid = R.groupnorm_ref(*args)[0]
            mb = R.bound(mid, R.groupnorm_cond(*args[:4])[0], R.C_GN, dt)
            emu = through(R.groupnorm_emu(*args)[0], dt) @ x['w'].t() + x['bias']
            assert R.worst(emu, R.head_ref(mid, x['w'], x['bias']), R.head_bound(mid, mb, x['w'], x['bias'])) <= 1
        for case in R.FUSED_CASES:
            x = R.map_inputs(case, dt)
            args = (x['x'], case.groups, x['gamma'], x['beta'], EPS, 2)
            mid = R.groupnorm_ref(*args)[0]
            mb = R.bound(mid, R.groupnorm_cond(*args[:4])[0], R.C_GN, dt)
            ref = R.dwconv5x5_ref(mid, x['taps'], case.H, case.W)
            emu = through(R.dwconv_emu(through(R.groupnorm_emu(*args)[0], dt), x['taps'], case.H, case.W), dt)
            assert R.worst(emu, ref, R.fused_bound(mid, mb, ref, x['taps'].double(), case.H, case.W, dt)) <= 1


# ------------------------------------------------------------------ mutations: each moves some element by more than 5x the bound
def gn_mut(name, dt, f32=False, images=1, act=0, mut_act=None, **mut):
    case = gn_case(name)
    x, g, b = R.gn_inputs(case, dt, f32, images)
    ref = R.groupnorm_ref(x, case.groups, g, b, EPS, act)
    return R.groupnorm_ref(x, case.groups, g, b, EPS, act if mut_act is None else mut_act, **mut), ref, R.bound(ref, R.groupnorm_cond(x, case.groups, g, b), R.C_GN, dt)


def rows_but(M, row):
    keep = torch.ones(M, dtype=torch.bool)
    keep[row] = False
    return keep


def m_neighbour(dt, delta):
    return gn_mut('rows-128', dt, swap=(0, 5, 32, delta))


def m_unclamped(dt):
    case = gn_case('rows-128')                 # fp32 input: with 16-bit input every sum over the constant group is exact
    x, g, b = R.gn_inputs(case, dt, True, 1)
    ref = R.groupnorm_ref(x, case.groups, g, b, EPS, 0)
    return through(R.groupnorm_emu(x, case.groups, g, b, EPS, 0, clamp=False), dt), ref, R.bound(ref, R.groupnorm_cond(x, case.groups, g, b), R.C_GN, dt)


def m_last_split_row(dt):
    case = gn_case('generic-empty-splits')
    assert R.gn_nonempty_splits(case.M) < R.GN_SPLITS
    return gn_mut(case.name, dt, stat_rows=rows_but(case.M, R.gn_nonempty_splits(case.M) * R.gn_split_rows(case.M) - 1))


def m_ln(dt, what):
    case = R.LN256_CASES[4]                       # M = 1674, fp32 a, 16-bit b
    x = R.ln256_inputs(case, dt)
    ln, lnp = R.layernorm_ref(x['a'], x['b'], x['gamma'], x['beta'], EPS, x['pos'])
    c, cp = R.layernorm_cond(x['a'], x['b'], x['gamma'], x['beta'], EPS, x['pos'])
    if what == 'b':
        return R.layernorm_ref(x['a'], None, x['gamma'], x['beta'])[0], ln, R.bound(ln, c, R.C_LN, dt)
    return ln, lnp, R.bound(lnp, cp, R.C_LN, dt)


def m_patch(dt, **mut):
    x = R.patch_inputs(128, 9, 11, 3)
    args = (x['x'], x['gamma'], x['beta'])
    ref = R.patch_merge_ref(*args)
    return R.patch_merge_ref(*args, **mut), ref, R.bound(ref, R.patch_merge_cond(*args), R.C_LN, dt)


def m_bilinear(dt, geom, ac, **mut):
    Hi, Wi, Ho, Wo = geom
    x = R.bilinear_inputs(Hi, Wi, 8, dt)
    ref = R.bilinear_ref(x, Ho, Wo, ac)
    return R.bilinear_ref(x, Ho, Wo, **mut), ref, R.bound(ref, R.bilinear_cond(x, Ho, Wo, ac), R.C_BILINEAR, dt)


def m_dwconv(dt):
    x, w = R.dwconv_inputs(9, 17, 24, dt)
    ref = R.dwconv5x5_ref(x, w, 9, 17)
    return R.dwconv5x5_ref(x, R.transpose_taps(w), 9, 17), ref, R.bound(ref, R.dwconv_cond(x, w, 9, 17), R.C_DOT, dt)


def exact(mutated, ref):
    """An exact operation: any difference is a failure, the bound is the smallest positive number."""
    return mutated.double(), ref.double(), torch.full(ref.shape, 5e-324, dtype=F64)


def m_pool(dt):
    x = R.pool_inputs(2, 5, 8, 1, dt, negative=True)
    return exact(R.maxpool3x3s2_ref(x, pad_value=0.0), R.maxpool3x3s2_ref(x))


def m_nearest(dt):
    src = seeded(951, (2, 13, 21))
    return exact(R.nearest_ref(src, 29, 47, rule='round'), R.nearest_ref(src, 29, 47))


def m_onehot(dt):
    lab = R.label_inputs(13, 21, 2)
    return exact(R.onehot16_ref(lab, 29, 47, 11, clear0=False), R.onehot16_ref(lab, 29, 47, 11))


UP = (7, 9, 61, 107)
MUTATIONS = {
    'statistics of group g+1 on one 8-channel vector': lambda dt: m_neighbour(dt, 1),
    'statistics of group g-1 on one 8-channel vector': lambda dt: m_neighbour(dt, -1),
    'statistics shared across images': lambda dt: gn_mut('rows-256', dt, images=3, share_images=True),
    'last row of M missing from the statistics': lambda dt: gn_mut('rows-128', dt, stat_rows=rows_but(333, 332)),
    'last row of the last non-empty split missing': m_last_split_row,
    'variance unclamped on a constant group': m_unclamped,
    'n = M * cpg off by one row': lambda dt: gn_mut('rows-128', dt, n_rows=332),
    'ReLU instead of none': lambda dt: gn_mut('rows-cpg8', dt, act=0, mut_act=1),
    'GELU instead of ReLU': lambda dt: gn_mut('rows-cpg8', dt, act=1, mut_act=2),
    'none instead of GELU': lambda dt: gn_mut('rows-cpg8', dt, act=2, mut_act=0),
    'GELU in its tanh form': lambda dt: gn_mut('rows-128', dt, act=2, mut_act=3),
    'b not added': lambda dt: m_ln(dt, 'b'),
    'pos not added': lambda dt: m_ln(dt, 'pos'),
    'patch-merge parts in [ee, eo, oe, oo] order': lambda dt: m_patch(dt, order=((0, 0), (0, 1), (1, 0), (1, 1))),
    'patch-merge odd border reads the neighbour': lambda dt: m_patch(dt, border='neighbour'),
    'bilinear with the other align_corners rule (True)': lambda dt: m_bilinear(dt, UP, True, align=False),
    'bilinear with the other align_corners rule (False)': lambda dt: m_bilinear(dt, UP, False, align=True),
    'bilinear i1 unclamped at the last row / column': lambda dt: m_bilinear(dt, UP, False, align=False, clamp_i1=False),
    'max-pool padding treated as 0': m_pool,
    'dwconv tap (dy, dx) transposed': m_dwconv,
    'nearest index with round instead of floor': m_nearest,
    'one-hot leaves channel 0 set under label 255': m_onehot,
}


@pytest.mark.parametrize('name', list(MUTATIONS))
def test_mutation_exceeds_five_times_the_bound(name):
    for dt in DTS:
        mutated, ref, bnd = MUTATIONS[name](dt)
        ratio = R.worst(mutated, ref, bnd)
        print(f'{name} [{str(dt)[6:]}]: worst |mutated - ref| / bound = {ratio:.3g}')
        assert ratio > 5, (name, dt, ratio)


# ------------------------------------------------------------------ coverage of the launch branches
def test_gpu_cases_reach_every_branch():
    cases = R.GN_CASES + (R.GN_CAP_CASE,)
    for f32 in (False, True):
        assert any(f == f32 for f, _ in R.GN_VARIANTS)
    # both branches; every case runs with 16-bit and with fp32 input (GN_VARIANTS)
    assert any(R.gn_rows_path(c.C) for c in cases) and any(not R.gn_rows_path(c.C) for c in cases)
    assert not R.gn_rows_path(192) and not R.gn_rows_path(320) and all(R.gn_rows_path(C) for C in (64, 128, 256, 512, 1024))
    for rows in (True, False):
        assert any(R.gn_rows_path(c.C) == rows and c.M < R.GN_SPLITS and R.gn_nonempty_splits(c.M) < R.GN_SPLITS for c in cases), rows
        assert any(R.gn_rows_path(c.C) == rows and R.gn_split_rows(c.M) > 1 for c in cases), rows
    assert any(R.gn_rows_path(c.C) and c.M % R.gn_apply_rows_per_wg(c.C) and c.M > R.gn_apply_rows_per_wg(c.C) for c in cases)
    assert any(c.groups == 64 for c in cases) and any(c.C // c.groups == 8 for c in cases) and any(c.C // c.groups == 24 for c in cases)
    assert R.gn_apply_passes(R.GN_CAP_CASE.M, R.GN_CAP_CASE.C) == 2 and all(R.gn_apply_passes(c.M, c.C) == 1 for c in R.GN_CASES)
    assert R.gn_apply_passes(R.GN_CAP_CASE.M - 56, R.GN_CAP_CASE.C) == 1         # "just over" the cap
    assert [R.stride_passes(n // 8, R.ADD16_CAP) for n in R.ADD_N] == [1, 2] and all(n % 8 == 0 for n in R.ADD_N)
    assert (R.ADD_N[1] // 8) % 256 and (R.ADD_N[1] // 8) % (256 * R.ADD16_CAP) < 256 * R.ADD16_CAP       # ragged tail in the second pass
    assert {p for p, n in R.ADD_GROUPED if R.stride_passes(n // 8, R.ADD16_GROUPED_CAP) == 2} == {1, 8}
    assert {c.M for c in R.LN256_CASES} == {1, 3, 5, 1674} and {c.b for c in R.LN256_CASES} == {None, '16', 'f32'}
    assert {c.a_f32 for c in R.LN256_CASES} == {True, False}
    g = R.EVICT_GEOM
    assert -(-g['He'] * g['We'] // 256) == 2 and g['He'] * g['We'] % 256 and g['keep'] < g['nc'] - 1
    assert any(H < 5 or W < 5 for H, W in R.MAPS) and all(H * W % 256 for H, W in R.LAYOUT_HW)
    assert all(Hd * Wd % 256 for _, _, Hd, Wd in R.NEAREST_GEOMS)


def test_gn_inputs_are_adversarial():
    """Every group has its own statistics up to the stated |mean| / std, one group is constant, normalised values span [-6, 6]."""
    zmin, zmax = 0.0, 0.0
    for f32 in (False, True):
        case = gn_case('rows-128')
        x, g, b = R.gn_inputs(case, BF16, f32, 1)
        v = x.view(1, case.M, case.groups, -1)
        mean, std = v.mean((1, 3))[0], v.std((1, 3))[0]
        ratio = (mean.abs() / std)[std > 0]
        assert ratio.max().item() > 0.7 * R.GN_RATIO[f32] and ratio.max().item() <= R.GN_RATIO[f32] * 1.01
        assert std[1].item() == 0 and len({round(s, 3) for s in std.tolist()}) >= 5
        z = R._gn_terms(x, case.groups, g, b, EPS)[2]
        zmin, zmax = min(zmin, z.min().item()), max(zmax, z.max().item())
    assert zmin < -6 and zmax > 6, (zmin, zmax)
