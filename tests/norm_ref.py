"""Plain float64 references of the normalisation / activation kernels (rmem_ocu_amd/csrc/norm_act.hip) and of the plain resampling
kernels at the top of rmem_ocu_amd/csrc/resample.hip, the per-element error bound the GPU tests hold those kernels to, fp32
emulations of the kernels' own formulas (the bound's constants are measured from them), a Python restatement of the GroupNorm / add
launch rules, and the seeded inputs of tests/test_hip_norm_resample.py.  No GPU, no library: torch and numpy only.

The bound, for an output stored in the element type dt:   |got - ref| <= ulp_dt(ref) + c_op * 2^-24 * cond_op   elementwise.
ulp_dt(ref) is the spacing of dt at |ref| (one whole unit: fp32 arithmetic may flip a rounding that, done exactly, errs by half a
unit); cond_op is the sum of the magnitudes of the reference's own terms, in float64, so c_op counts fp32 roundings.  fp32 outputs
have no ulp term.  Pure data movement (max-pool, layout changes, nearest resize, one-hot, add) is compared with torch.equal.

tests/test_norm_ref_host.py checks, on the CPU, the references against torch's own operators, the emulations against the bound, every
mutation of the issue's list against 5x the bound, and the GPU case list against the branches it is meant to reach."""
import math
from collections import namedtuple

import numpy as np
import torch

from gated_ref import dwconv5x5_ref, through            # noqa: F401  (dwconv5x5_ref is part of this module's references)
from test_hip_ops import seeded

F32, F64 = torch.float32, torch.float64
BF16, F16 = torch.bfloat16, torch.float16
DTS = (BF16, F16)
EPS = 1e-5
U24 = 2.0 ** -24
SENTINEL = -777.0                                        # exact in bfloat16, IEEE half and fp32; no case produces it

# ------------------------------------------------------------------ the bound
_MANT = {BF16: 7, F16: 10}
_EMIN = {BF16: -126, F16: -14}


def ulp(ref, dt):
    """Spacing of dt at |ref| (float64): 2^(e - mantissa bits) in the binade [2^e, 2^(e+1)) of |ref|, the subnormal spacing below."""
    r = ref.to(F64).abs()
    e = torch.frexp(r)[1] - 1
    e = torch.where(r == 0, torch.full_like(e, _EMIN[dt]), e).clamp_min(_EMIN[dt])
    return torch.ldexp(torch.ones_like(r), e - _MANT[dt])


def bound(ref, cond, c, dt=None):
    """ulp_dt(ref) + c * 2^-24 * cond; dt None: an fp32 output, no ulp term."""
    b = c * U24 * cond.to(F64)
    return b if dt is None else b + ulp(ref, dt)


def worst(got, ref, bnd):
    """max over elements of |got - ref| / bound (inf where got is not finite)."""
    got = got.detach().to(device='cpu', dtype=F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return math.inf
    return ((got - ref).abs() / bnd).max().item()


def needed_c(got, ref, cond, dt=None):
    """The smallest c with which got meets bound(ref, cond, c, dt)."""
    err = (got.to(F64) - ref).abs()
    if dt is not None:
        err = (err - ulp(ref, dt)).clamp_min(0)
    m = err > 0
    return (err[m] / (U24 * cond.to(F64)[m])).max().item() if m.any() else 0.0


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def c_from(measured):
    """4x the measured constant, rounded up to a power of two (the margin: the GPU's own summation order, fma contraction and its
    approximate rcp / exp2); never below 1, fp32 arithmetic rounds at least once."""
    return max(1.0, pow2_ceil(4 * measured)) if measured > 0 else 1.0


# measured: the largest needed_c of the fp32 emulation below over all of this file's cases (test_norm_ref_host.py re-measures it and
# fails if a case needs more than the value written here); chosen: c_from(measured)
MEASURED_C_LN, C_LN = 12.9, 64.0            # ln128, M = 333, fp32 in and out: a row whose mean is ~0, where |mean| hides sum |v| / C
MEASURED_C_GN, C_GN = 2.87, 16.0            # 64 groups of 8 channels, fp32 input at |mean| / std = 32
MEASURED_C_DOT, C_DOT = 3.26, 16.0          # the head's 128-long fp32 product (the 25 depth-wise taps need less)
MEASURED_C_BILINEAR, C_BILINEAR = 0.73, 4.0
MEASURED_C_EVICT, C_EVICT = 0.39, 2.0


# ------------------------------------------------------------------ activations
def act_ref(f, act):
    """0 none, 1 ReLU, 2 GELU in its exact erf form; 3 (mutation checks only): GELU's tanh form."""
    if act == 1:
        return f.clamp_min(0)
    if act == 2:
        return 0.5 * f * (1 + torch.erf(f / math.sqrt(2)))
    if act == 3:
        return 0.5 * f * (1 + torch.tanh(math.sqrt(2 / math.pi) * (f + 0.044715 * f ** 3)))
    return f


def gelu_emu(x):
    """gelu_erf of norm_act.hip in fp32: erf from Abramowitz-Stegun 7.1.26, fp32 reciprocal and exp2."""
    x = x.to(F32)
    z = x.abs() * np.float32(0.70710678118654752)
    t = 1 / (np.float32(0.3275911) * z + 1)
    q = np.float32(1.061405429) * t + np.float32(-1.453152027)
    for k in (1.421413741, -0.284496736, 0.254829592):
        q = q * t + np.float32(k)
    erfc = q * t * torch.exp2(z * z * np.float32(-1.4426950408889634))
    return np.float32(0.5) * x * torch.where(x < 0, erfc, 2 - erfc)


def act_emu(f, act):
    return f.clamp_min(0) if act == 1 else gelu_emu(f) if act == 2 else f


# ------------------------------------------------------------------ LayerNorm
def _ln_terms(a, b, gamma, beta, eps):
    v = a.to(F64) if b is None else a.to(F64) + b.to(F64)
    mean = v.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + eps)
    g, bt = gamma.to(F64), beta.to(F64)
    return (v - mean) * rstd * g + bt, (v.abs() + mean.abs()) * rstd * g.abs() + bt.abs()


def layernorm_ref(a, b, gamma, beta, eps=EPS, pos=None):
    """(ln, ln + pos) in float64: ln = LayerNorm(a + b) over the last dimension, biased variance (b, pos may be None)."""
    ln = _ln_terms(a, b, gamma, beta, eps)[0]
    return ln, None if pos is None else ln + pos.to(F64)


def layernorm_cond(a, b, gamma, beta, eps=EPS, pos=None):
    """cond of (ln, ln + pos): (|v| + |mean|) * rstd * |gamma| + |beta| (+ |pos|)."""
    c = _ln_terms(a, b, gamma, beta, eps)[1]
    return c, None if pos is None else c + pos.to(F64).abs()


def wave_sum_emu(v):
    """Sum over the last dimension the way one wave does it, in fp32: 64 lanes of consecutive channels, each summed in order, then
    the xor butterfly (lane i + lane i ^ 32, then ^ 16, ... ^ 1)."""
    s = torch.zeros(*v.shape[:-1], 64, dtype=F32)
    for j in range(v.shape[-1] // 64):
        s = s + v.reshape(*v.shape[:-1], 64, -1)[..., j]
    for o in (32, 16, 8, 4, 2, 1):
        s = s[..., :o] + s[..., o:2 * o]
    return s


def layernorm_emu(a, b, gamma, beta, eps=EPS, pos=None):
    """The kernels' formula in fp32: sum, centre, then square (rmem_ln256_row / k_layernorm_c) -> (ln, ln + pos)."""
    v = a.to(F32) if b is None else a.to(F32) + b.to(F32)
    inv = np.float32(1.0 / v.shape[-1])
    d = v - wave_sum_emu(v) * inv
    rstd = torch.rsqrt(wave_sum_emu(d * d) * inv + np.float32(eps))
    o = d * rstd * gamma.to(F32) + beta.to(F32)
    return o, None if pos is None else o + pos.to(F32)


PATCH_ORDER = ((0, 0), (1, 0), (0, 1), (1, 1))           # (row, col) parity of the four parts: [ee, oe, eo, oo]


def patch_gather(x, order=PATCH_ORDER, border='zero'):
    """[images, H, W, C] -> [images, ceil(H/2) * ceil(W/2), 4C]: the 2x2 neighbourhood of every output token, zeros beyond an odd
    border.  order / border='neighbour' (mutation checks only): another part order; the last row / column read again instead of zero."""
    images, H, W, C = x.shape
    Hp, Wp = H + H % 2, W + W % 2
    xp = torch.zeros(images, Hp, Wp, C, dtype=x.dtype)
    xp[:, :H, :W] = x
    if border == 'neighbour':
        xp[:, H:, :W] = x[:, H - 1:H]
        xp[:, :, W:] = xp[:, :, W - 1:W]
    return torch.cat([xp[:, r::2, c::2] for r, c in order], -1).reshape(images, -1, 4 * C)


def patch_merge_ref(x, gamma, beta, eps=EPS, **mut):
    """Swin patch merging's gather + LayerNorm over 4C, float64."""
    return layernorm_ref(patch_gather(x.to(F64), **mut), None, gamma, beta, eps)[0]


def patch_merge_cond(x, gamma, beta, eps=EPS):
    return layernorm_cond(patch_gather(x.to(F64)), None, gamma, beta, eps)[0]


def patch_merge_emu(x, gamma, beta, eps=EPS):
    return layernorm_emu(patch_gather(x.to(F32)), None, gamma, beta, eps)[0]


# ------------------------------------------------------------------ GroupNorm
GN_SPLITS = 64


def _gn_terms(x, groups, gamma, beta, eps, stat_rows=None, n_rows=None, share_images=False, swap=None):
    x = x.to(F64)
    images, M, C = x.shape
    cpg = C // groups
    xs = (x if stat_rows is None else x[:, stat_rows]).reshape(images, -1, groups, cpg)
    n = (M if n_rows is None else n_rows) * cpg
    s, ss = xs.sum((1, 3)), (xs * xs).sum((1, 3))
    if share_images:
        s, ss, n = s.sum(0, keepdim=True).expand(images, -1), ss.sum(0, keepdim=True).expand(images, -1), n * images
    mean = s / n
    if stat_rows is None and n_rows is None and not share_images:
        var = ((xs - mean[:, None, :, None]) ** 2).mean((1, 3))              # two passes: no cancellation in the reference
    else:
        var = (ss / n - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    me = mean.repeat_interleave(cpg, 1)[:, None, :].expand(images, M, C).clone()
    re = rstd.repeat_interleave(cpg, 1)[:, None, :].expand(images, M, C).clone()
    ve = var.repeat_interleave(cpg, 1)[:, None, :].expand(images, M, C)
    if swap is not None:
        im, row, c0, delta = swap
        g = c0 // cpg + delta
        me[im, row, c0:c0 + 8], re[im, row, c0:c0 + 8] = mean[im, g], rstd[im, g]
    g, bt = gamma.to(F64), beta.to(F64)
    z = (x - me) * re
    cond = (x.abs() + me.abs()) * re * g.abs() + bt.abs() + (1 + me * me / (ve + eps)) * (z * g).abs()
    return z * g + bt, cond, z


def groupnorm_ref(x, groups, gamma, beta, eps=EPS, act=0, **mut):
    """act(GroupNorm(x)) of x [images, M, C] in float64: statistics per image and group over M x C/groups values, biased variance.
    act: see act_ref.  Keyword arguments are for the mutation checks only: stat_rows (bool [M]: the rows the statistics see, n
    unchanged), n_rows (the row count the sums are divided by), share_images (one set of statistics for all images), swap (image, row,
    c0, delta): the 8 channels from c0 of that row use the statistics of group + delta.

    Envelope: the kernels form the variance in one pass, E[x^2] - E[x]^2 in fp32, whose absolute error grows with mean^2; the cases
    here go up to |mean| / std = 32 with fp32 input and 8 with 16-bit input (whose own rounding already limits what a larger
    offset could carry), and cond's statistics term (1 + mean^2 / (var + eps)) |z gamma| is what covers that cancellation."""
    return act_ref(_gn_terms(x, groups, gamma, beta, eps, **mut)[0], act)


def groupnorm_cond(x, groups, gamma, beta, eps=EPS):
    """(|x| + |mean|) rstd |gamma| + |beta| + (1 + mean^2 / (var + eps)) |z gamma|; the same for every activation (ReLU and GELU
    are at most 1.13-Lipschitz, and the erf polynomial's 1.5e-7 is relative to |pre| / 2: both are left to c)."""
    return _gn_terms(x, groups, gamma, beta, eps)[1]


def gn_stats_emu(x, groups, eps=EPS, clamp=True):
    """(mean, rstd) [images, groups] the way the kernels get them, in fp32: (sum, sum of squares) per split of ceil(M / 64) rows,
    then gn_finalize: four quarters of 16 splits summed in order, (q0 + q1) + (q2 + q3), var = max(ss / n - mean^2, 0)."""
    x = x.to(F32)
    images, M, C = x.shape
    cpg, rp = C // groups, gn_split_rows(M)
    xp = torch.zeros(images, GN_SPLITS * rp, C, dtype=F32)
    xp[:, :M] = x
    xp = xp.view(images, GN_SPLITS, rp, groups, cpg)
    part = torch.stack([xp.sum((2, 4)), (xp * xp).sum((2, 4))])                # [2, images, 64, groups]
    part = part.view(2, images, 4, GN_SPLITS // 4, groups)                     # split = 16 * quarter + i
    q = torch.zeros(2, images, 4, groups, dtype=F32)
    for i in range(GN_SPLITS // 4):
        q = q + part[:, :, :, i]
    tot = (q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3])
    n = np.float32(M) * np.float32(cpg)
    mean = tot[0] / n
    var = tot[1] / n - mean * mean
    if clamp:
        var = var.clamp_min(0)
    return mean, torch.rsqrt(var + np.float32(eps))


def groupnorm_emu(x, groups, gamma, beta, eps=EPS, act=0, clamp=True):
    """k_gn_apply's formula in fp32 on gn_stats_emu's statistics (before the store's rounding to the element type)."""
    cpg = x.shape[2] // groups
    mean, rstd = gn_stats_emu(x, groups, eps, clamp)
    f = (x.to(F32) - mean.repeat_interleave(cpg, 1)[:, None]) * rstd.repeat_interleave(cpg, 1)[:, None] * gamma.to(F32) + beta.to(F32)
    return act_emu(f, act)


# ------------------------------------------------------------------ products after a GroupNorm (head, fused depth-wise conv)
def head_ref(mid, w, bias):
    """mid [.., C] (float64, the GroupNorm reference) @ w[N, C]^T + bias."""
    return mid @ w.to(F64).t() + (0 if bias is None else bias.to(F64))


def head_bound(mid, mid_bound, w, bias, c=None):
    """The head stores act(GroupNorm) in the element type before its product, so every term carries the GroupNorm bound (ulp term
    included) times |w|; the fp32 product itself adds c * 2^-24 * (sum |mid w| + |bias|).  The output is fp32."""
    c = C_DOT if c is None else c
    wa = w.to(F64).abs()
    return mid_bound @ wa.t() + c * U24 * (mid.abs() @ wa.t() + (0 if bias is None else bias.to(F64).abs()))


def dwconv_cond(x, w, H, W):
    """sum |x w| over the taps."""
    return dwconv5x5_ref(x.to(F64).abs(), w.to(F64).abs(), H, W)


def dwconv_emu(x, w, H, W):
    """k_dwconv5's fp32 accumulation, dx outer and dy inner."""
    C = x.shape[1]
    xp = torch.zeros(H + 4, W + 4, C, dtype=F32)
    xp[2:H + 2, 2:W + 2] = x.to(F32).view(H, W, C)
    y = torch.zeros(H, W, C, dtype=F32)
    for dx in range(5):
        for dy in range(5):
            y = y + xp[dy:dy + H, dx:dx + W] * w[dy * 5 + dx].to(F32)
    return y.view(H * W, C)


def fused_bound(mid, mid_bound, ref, w, H, W, dt, c=None):
    """GroupNorm + activation + depth-wise 5x5: as head_bound, over the 25 taps, plus the ulp of the stored result."""
    c = C_DOT if c is None else c
    return dwconv5x5_ref(mid_bound, w.abs(), H, W) + bound(ref, dwconv_cond(mid, w, H, W), c, dt)


def transpose_taps(w):
    """w [25, C] with tap (dy, dx) <-> (dx, dy) (mutation checks only)."""
    return w.view(5, 5, -1).transpose(0, 1).reshape(25, -1)


# ------------------------------------------------------------------ max-pool, bilinear, nearest, one-hot, eviction scores
def maxpool3x3s2_ref(x, pad_value=-math.inf):
    """x [images, H, W, C] -> [images, ceil(H/2), ceil(W/2), C]: 3x3 window, stride 2, padding 1; the padding never wins
    (pad_value 0: mutation checks only)."""
    images, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((images, 2 * Ho + 1, 2 * Wo + 1, C), pad_value, dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x.to(F64)
    out = torch.full((images, Ho, Wo, C), -math.inf, dtype=F64)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2])
    return out


def src_coord(n_in, n_out, align, clamp_i1=True):
    """(i0, i1, w1) of every destination index: PyTorch's upsample_bilinear2d rule, the coordinate in fp32 as ATen and the kernels
    compute it (rmem_src_coord; its fused multiply-add is one rounding of the exact product and sum, as float64 holds them here).
    clamp_i1 False (mutation checks only): i1 = i0 + 1 even beyond the last row / column."""
    d = np.arange(n_out, dtype=np.float32)
    if align:
        s = d * (np.float32(n_in - 1) / np.float32(n_out - 1)) if n_out > 1 else np.zeros(n_out, np.float32)
    else:
        s = np.maximum(((d.astype(np.float64) + 0.5) * np.float64(np.float32(n_in) / np.float32(n_out)) - 0.5).astype(np.float32), np.float32(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1) if clamp_i1 else i0 + 1
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy((s - i0.astype(np.float32)).astype(np.float64))


def bilinear_ref(x, Ho, Wo, align, clamp_i1=True, dtype=F64):
    """x [images, Hi, Wi, C] -> [images, Ho, Wo, C]: the blend of the four taps in float64 (dtype F32: the kernel's fp32 blend,
    rmem_bilerp without its fused multiply-adds).  Beyond the map (clamp_i1 False only) the taps are zero."""
    images, Hi, Wi, C = x.shape
    y0, y1, wy = src_coord(Hi, Ho, align, clamp_i1)
    x0, x1, wx = src_coord(Wi, Wo, align, clamp_i1)
    xp = torch.zeros(images, Hi + 1, Wi + 1, C, dtype=dtype)
    xp[:, :Hi, :Wi] = x.to(dtype)
    wy, wx = wy.to(dtype)[None, :, None, None], wx.to(dtype)[None, None, :, None]
    top = xp[:, y0][:, :, x0] * (1 - wx) + xp[:, y0][:, :, x1] * wx
    bot = xp[:, y1][:, :, x0] * (1 - wx) + xp[:, y1][:, :, x1] * wx
    return top * (1 - wy) + bot * wy


def bilinear_cond(x, Ho, Wo, align):
    """The blend of |taps|."""
    return bilinear_ref(x.abs(), Ho, Wo, align)


def nearest_index(n_in, n_out, rule='floor'):
    """F.interpolate(mode='nearest'): min(floor(d * (in / out)), in - 1) with the scale and the product in fp32.
    rule 'round' (mutation checks only) / 'f64' (the same rule in float64: where fp32 differs is what NEAREST_PAIR names)."""
    d = np.arange(n_out)
    if rule == 'f64':
        return torch.from_numpy(np.minimum(d * n_in // n_out, n_in - 1))
    s = d.astype(np.float32) * (np.float32(n_in) / np.float32(n_out))
    s = np.floor(s) if rule == 'floor' else np.round(s)
    return torch.from_numpy(np.minimum(s.astype(np.int64), n_in - 1))


def nearest_ref(src, Hd, Wd, flip=False, rule='floor'):
    """src [..., Hs, Ws] -> [..., Hd, Wd]: nearest resize of the (optionally mirrored along W) source."""
    Hs, Ws = src.shape[-2:]
    if flip:
        src = src.flip(-1)
    return src[..., nearest_index(Hs, Hd, rule), :][..., nearest_index(Ws, Wd, rule)]


def onehot16_ref(label, Hd, Wd, ncls, rule='floor', clear0=True):
    """label [images, Hs, Ws] -> fp32 [images, Hd * Wd, 16]: nearest resize, channels 0..ncls-1 one-hot, channel ncls = 1 where the
    label is 255 (the ignore label sets no class channel; ids >= ncls other than 255 set nothing).
    clear0 False (mutation checks only): label 255 leaves channel 0 set, as an `else background` would."""
    lab = nearest_ref(label, Hd, Wd, rule=rule).long().reshape(label.shape[0], Hd * Wd)
    out = torch.zeros(*lab.shape, 16, dtype=F32)
    for c in range(ncls):
        out[..., c] = (lab == c).float()
    out[..., ncls] = (lab == 255).float()
    if not clear0:
        out[..., 0] += (lab == 255).float()
    return out


def _evict_terms(logits, mass, keep, He, We, dtype):
    lg = logits.to(dtype).clone()
    lg[..., keep + 1:] = -1.0e10
    v = bilinear_ref(lg[None], He, We, True, dtype=dtype)[0].reshape(He * We, -1)
    v[:, keep + 1:] = -1.0e10
    fg = 1 - torch.softmax(v, -1)[:, 0]
    return (mass.to(dtype) * fg[:, None]).sum(0), v


def evict_ref(logits, mass, keep, He, We):
    """scores[t] = sum_q mass[q, t] * (1 - softmax(bilinear_ac(logits with ids > keep masked to -1e10))[0]), float64.
    logits [Hi, Wi, nc], mass [He * We, T]."""
    return _evict_terms(logits, mass, keep, He, We, F64)[0]


def evict_cond(logits, mass, keep, He, We):
    """sum_q |mass| * (1 + the blend of |taps| of the kept channels, their maximum): the foreground probability moves by at most
    the error of its logits."""
    lg = logits.to(F64).abs()[..., :keep + 1]
    amp = bilinear_ref(lg[None], He, We, True)[0].reshape(He * We, -1).amax(-1)
    return (mass.to(F64).abs() * (1 + amp)[:, None]).sum(0)


def evict_emu(logits, mass, keep, He, We):
    return _evict_terms(logits, mass, keep, He, We, F32)[0]


# ------------------------------------------------------------------ the launch rules, restated (norm_act.hip)
def gn_rows_path(C):
    """gn_launch_stats / gn_launch_apply take the row-coalesced kernels iff a row's 16-byte vectors tile the 256 threads."""
    vpr = C // 8
    return vpr <= 256 and 256 % vpr == 0


def gn_split_rows(M):
    """Rows per statistics split: 64 splits of ceil(M / 64) rows, the last ones empty when M is small."""
    return -(-M // GN_SPLITS)


def gn_nonempty_splits(M):
    return -(-M // gn_split_rows(M))


def gn_apply_rows_per_wg(C):
    """k_gn_apply_rows: 8 rows per thread, 256 / (C/8) row lanes."""
    return 8 * (256 // (C // 8))


ADD16_CAP, ADD16_GROUPED_CAP, GN_APPLY_CAP = 2048, 1024, 2048       # blocks of 256 threads x 8 elements


def stride_passes(vectors, cap):
    """Iterations of the grid-stride loop of a kernel launched with min(cap, ceil(vectors / 256)) blocks of 256 threads."""
    blocks = min(cap, -(-vectors // 256))
    return -(-vectors // (blocks * 256))


def gn_apply_passes(M, C):
    """Grid-stride passes of the generic k_gn_apply (1 on the rows path, which has no such loop)."""
    return 1 if gn_rows_path(C) else stride_passes(M * (C // 8), GN_APPLY_CAP)


# ------------------------------------------------------------------ the cases of tests/test_hip_norm_resample.py
GnCase = namedtuple('GnCase', 'name M C groups seed')
GN_CASES = (
    GnCase('generic-cpg24', 150, 192, 8, 8100),
    GnCase('generic-empty-splits', 40, 320, 8, 8110),
    GnCase('rows-128', 333, 128, 8, 8120),
    GnCase('rows-256', 70, 256, 32, 8130),
    GnCase('rows-1024', 65, 1024, 32, 8140),
    GnCase('rows-cpg8', 9, 64, 8, 8150),
    GnCase('rows-64-groups', 130, 512, 64, 8160),
)
GN_CAP_CASE = GnCase('generic-grid-cap', 21901, 192, 8, 8170)         # 21901 * 24 vectors > 2048 * 256: a second grid-stride pass
GN_VARIANTS = ((False, 1), (False, 3), (True, 1))                     # (fp32 input, images)
GN_RATIO = {False: 8.0, True: 32.0}                                   # largest |mean| / std of a group: 16-bit input, fp32 input
GN_CONST = {False: 100.5, True: 100.7}      # the constant group's value: exact in both element types (every sum is then exact too) /
                                            # fp32 input: not exact, the one-pass variance comes out of rounding errors alone


GN_CONST_MAX_M = 1024                       # the grid-cap case has no constant group: the output there is the fp32 error of a sum of
                                            # half a million equal addends times 1 / sqrt(eps), which measures the sum, not the kernel


def gn_outlier_rows(M):
    """(the last row of M, the last row of the first statistics split)."""
    return M - 1, gn_split_rows(M) - 1


def gn_inputs(case, dt, in_f32, images):
    """x [images, M, C] (fp32; rounded through dt unless in_f32), gamma, beta [C].  Every (image, group) has its own scale
    (1/8 .. 8) and its own mean (-R .. R standard deviations, R = GN_RATIO); group 1 of image 0 is constant (M <= GN_CONST_MAX_M); the last row of M
    sits 4 deviations above its group's mean and the last row of the first split 4 below; single elements at the map's corners
    sit 7 deviations out."""
    M, C, groups = case.M, case.C, case.groups
    cpg = C // groups
    k = torch.arange(images * groups).view(images, groups)
    sigma = 2.0 ** ((k * 5) % 7 - 3).float()
    mean = (GN_RATIO[in_f32] * (((k * 7) % 9).float() / 4 - 1) * sigma)[:, None, :, None]
    sigma = sigma[:, None, :, None]
    x = seeded(case.seed + images, (images, M, groups, cpg)) * sigma + mean
    hi, lo = gn_outlier_rows(M)
    if lo != hi:
        x[:, lo] = (mean - 4 * sigma)[:, 0]
    x[:, hi] = (mean + 4 * sigma)[:, 0]
    x[:, 0, :, cpg - 1] = (mean + 7 * sigma)[:, 0, :, 0]
    x[:, M // 2, :, 0] = (mean - 7 * sigma)[:, 0, :, 0]
    if M <= GN_CONST_MAX_M:
        x[0, :, 1] = GN_CONST[in_f32]
    x = x.reshape(images, M, C)
    gamma = 1 + 0.25 * seeded(case.seed + 50, (C,))
    beta = 0.25 * seeded(case.seed + 51, (C,))
    return (x if in_f32 else through(x, dt)), gamma, beta


Ln256Case = namedtuple('Ln256Case', 'M a_f32 b seed')                 # b: None, '16' or 'f32'
LN256_CASES = tuple(Ln256Case(M, a, b, 8200 + 10 * i) for i, (M, a, b) in enumerate(
    [(1, True, None), (3, False, '16'), (5, True, 'f32'), (5, False, None), (1674, True, '16'), (1674, False, 'f32')]))
LN256_LD = dict(lda=768, ldb=512, ldy=1024, ycol=256, ldyp=512, ldyf=260)


def ln_rows(seed, M, C, dt, f32):
    """[M, C] rows, each with its own mean and scale; row 0 has mean 30 and deviation 0.5 (fp32 input only: 16-bit input cannot
    carry that offset); the last row of M >= 3 is constant."""
    k = torch.arange(M, dtype=F32)[:, None]
    x = seeded(seed, (M, C)) * 2.0 ** ((k * 3) % 5 - 2) + ((k * 7) % 11 - 5) * 0.5
    if f32:
        x[0] = seeded(seed + 1, (C,)) * 0.5 + 30
    if M >= 3:
        x[M - 1] = 2.5
    return x if f32 else through(x, dt)


def ln256_inputs(case, dt):
    """a, b (or None), gamma, beta, pos: fp32 values, 16-bit operands rounded through dt."""
    a = ln_rows(case.seed, case.M, 256, dt, case.a_f32)
    b = None if case.b is None else ln_rows(case.seed + 2, case.M, 256, dt, case.b == 'f32')
    if b is not None and case.a_f32 and case.b == 'f32':
        b[0] = seeded(case.seed + 3, (256,)) * 0.5                     # keep row 0 at mean 30, deviation < 1
    return dict(a=a, b=b, gamma=1 + 0.25 * seeded(case.seed + 4, (256,)), beta=0.25 * seeded(case.seed + 5, (256,)),
                pos=seeded(case.seed + 6, (case.M, 256)))


LN_GENERIC_C, LN_GENERIC_M = (128, 256, 512, 1024), (1, 6, 333)


def ln_generic_inputs(C, M, dt, a_f32):
    seed = 8300 + C + M
    return dict(a=ln_rows(seed, M, C, dt, a_f32), gamma=1 + 0.25 * seeded(seed + 4, (C,)), beta=0.25 * seeded(seed + 5, (C,)))


PATCH_C, PATCH_HW, PATCH_IMAGES = (128, 256), ((1, 1), (2, 3), (7, 7), (9, 11), (6, 8)), (1, 3)


def patch_inputs(C, H, W, images):
    """x [images, H, W, C] fp32: every image and every pixel parity has its own offset, the last row / column pixel is an outlier."""
    seed = 8400 + C + 16 * H + W
    x = seeded(seed, (images, H, W, C))
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    x = x + ((yy % 2) * 2.0 - (xx % 2) * 1.0)[None, :, :, None] + torch.arange(images, dtype=F32)[:, None, None, None] * 0.75
    x[:, H - 1, W - 1] += 6.0
    return dict(x=x, gamma=1 + 0.25 * seeded(seed + 1, (4 * C,)), beta=0.25 * seeded(seed + 2, (4 * C,)))


MAPS = ((1, 7), (3, 2), (8, 16), (9, 17), (11, 13))                    # H x W of the head / depth-wise cases, some below the 5x5 filter
MapCase = namedtuple('MapCase', 'H W C groups seed')
HEAD_CASES = tuple(MapCase(H, W, 128, 8, 8500 + i) for i, (H, W) in enumerate(MAPS))          # the head is C = 128 only
FUSED_CASES = tuple(MapCase(H, W, C, 8, 8520 + 8 * i + C // 64) for i, (H, W) in enumerate(MAPS) for C in (64, 128))
DWCONV_C = (8, 24, 64)
HEAD_N = 11


def map_inputs(case, dt, images=1):
    """gn_inputs of an H x W map (16-bit input), plus the head's w [11, C] (rounded through dt), bias and the depth-wise taps [25, C]."""
    x, gamma, beta = gn_inputs(GnCase('map', case.H * case.W, case.C, case.groups, case.seed), dt, False, images)
    return dict(x=x, gamma=gamma, beta=beta, w=through(seeded(case.seed + 60, (HEAD_N, case.C), case.C ** -0.5), dt),
                bias=0.1 * seeded(case.seed + 61, (HEAD_N,)), taps=seeded(case.seed + 62, (25, case.C), 0.2))


def dwconv_inputs(H, W, C, dt):
    seed = 8600 + 32 * H + W + C
    x = seeded(seed, (H * W, C)) + torch.arange(H * W, dtype=F32)[:, None] % 3
    x[H * W - 1] += 5.0
    return through(x, dt), seeded(seed + 1, (25, C), 0.2)


ADD_N = (8, 8 * (256 * ADD16_CAP) + 8 * 259)                          # one vector; a second grid-stride pass with a ragged tail
ADD_GROUPED = ((1, 8 * (256 * ADD16_GROUPED_CAP) + 8 * 259), (8, 8 * (256 * ADD16_GROUPED_CAP) + 8 * 259), (3, 8))   # (problems, n)

POOL_HW, POOL_C, POOL_IMAGES = ((1, 1), (2, 2), (2, 5), (48, 64), (49, 65)), (8, 64), (1, 2)


def pool_inputs(H, W, C, images, dt, negative=False):
    """x [images, H, W, C] rounded through dt; negative: every value below zero (a zero padding would win every border window)."""
    x = seeded(8700 + 8 * H + W + C + images, (images, H, W, C))
    return through(-x.abs() - 0.5 if negative else x, dt)


BILINEAR_GEOMS = ((1, 1, 5, 7), (1, 9, 4, 9), (31, 54, 31, 54), (31, 54, 16, 27), (5, 6, 1, 1), (7, 9, 61, 107))   # Hi, Wi, Ho, Wo
BILINEAR_C = (8, 136)


def bilinear_inputs(Hi, Wi, C, dt, images=1):
    """x [images, Hi, Wi, C] rounded through dt: a ramp per row and column under the noise, the last row and column lifted."""
    x = seeded(8800 + 64 * Hi + Wi + C, (images, Hi, Wi, C))
    x = x + torch.arange(Hi, dtype=F32)[None, :, None, None] * 0.5 - torch.arange(Wi, dtype=F32)[None, None, :, None] * 0.25
    x[:, Hi - 1] += 3.0
    x[:, :, Wi - 1] -= 3.0
    return through(x, dt)


# (in, out) of a nearest resize with a non-integer ratio where fp32 floor(d * (in / out)) is not the exact floor(d * in / out) for
# some d (14 / 46 = 7 / 23: at d = 23 the fp32 product falls below 7).  test_norm_ref_host.py asserts it.
NEAREST_PAIR = (14, 46)
NEAREST_GEOMS = ((13, 21, 29, 47), (14, 26, 46, 22), (30, 50, 17, 23), (6, 9, 6, 9))        # Hs, Ws, Hd, Wd; Hd * Wd % 256 != 0
LAYOUT_HW = ((1, 1), (17, 19), (33, 31))                                                # H * W % 256 != 0, one of them > 256


def label_inputs(Hs, Ws, images, ncls=11):
    """uint8-valued labels [images, Hs, Ws]: ids 0..ncls-1, a patch of 255, a patch of ids >= ncls, background corner."""
    g = torch.Generator().manual_seed(8900 + Hs * 64 + Ws)
    lab = torch.randint(0, ncls, (images, Hs, Ws), generator=g)
    lab[:, : max(1, Hs // 3), : max(1, Ws // 3)] = 255
    lab[:, -1, -max(1, Ws // 4):] = ncls + 2
    lab[:, Hs // 2, Ws // 2] = 0
    return lab


EVICT_GEOM = dict(Hi=25, Wi=33, He=17, We=19, nc=11, keep=6)           # 323 tokens: two blocks, the second ragged; keep < nc - 1
EVICT_T = (1, 5, 32)


def evict_inputs(T):
    """logits [Hi, Wi, nc] (the masked ids carry large values: leaving them in changes every score), mass [He * We, T] >= 0 with one
    heavy token in the ragged second block."""
    g = EVICT_GEOM
    lg = seeded(9000, (g['Hi'], g['Wi'], g['nc'])) * 3.0
    lg[..., g['keep'] + 1:] += 20.0
    mass = seeded(9001 + T, (g['He'] * g['We'], T)).abs()
    mass[g['He'] * g['We'] - 1] += 10.0
    return lg, mass


SCATTER_CLIPS, SCATTER_L, SCATTER_C = 3, 143, 256
SCATTER_BLOCKS = (16, SCATTER_L * SCATTER_C * 2)                       # bytes: one 16-byte unit; L rows of C 16-bit values
