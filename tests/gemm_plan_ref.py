"""Plain-Python restatement of the GEMM launch plan of rmem_ocu_amd/csrc/gemm_conv.hip: which kernel family, ring depth, split
count and grid a convolution / linear shape gets.  Written from the dispatcher the plan function replaced (the branches of
rmem_conv2d_nhwc, rmem_conv1x1_dual_nhwc and rmem_linear_grouped at their default knobs plus RMEM_GEMM_PC), not from the plan
function, so tests/test_gemm_plan_host.py compares two independent statements of the same rules.  No GPU, no library."""

GENERAL64, SCALAR64, ROWRUN64, ONE128, PC128, ROWRUN128, DUAL64, DUAL128, GROUPED = range(9)
FAMILY_NAMES = ('general64', 'scalar64', 'rowrun64', 'one128', 'pc128', 'rowrun128', 'dual64', 'dual128', 'grouped')
CONV2D, DUAL, LINEAR_GROUPED = range(3)
FIELDS = ('family', 'tile', 'ring', 'is1x1', 'fast', 'splits', 'steps_per_split', 'xcd_ny', 'grid_x', 'grid_y', 'grid_z', 'threads')


def cdiv(a, b):
    return -(-a // b)


def out_size(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def fast_form(H, W, Cin, Cout, KH, KW, stride, pad, batch, ldx=0):
    """0: general form, 1: scalar k-walk (Cin % 64 == 0, <= 32 taps), 2: row-run; 1 and 2 need operands below 2 GB."""
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    M, K = batch * Ho * Wo, KH * KW * Cin
    is1x1 = KH == 1 and KW == 1 and stride == 1 and pad == 0
    x_elems = (M - 1) * (ldx or Cin) + Cin if is1x1 else batch * H * W * Cin
    shift = 0 if is1x1 else (pad * W + pad) * Cin
    lim = (1 << 31) - (1 << 22)
    if not ((x_elems + shift) * 2 < lim and Cout * K * 2 < lim):
        return 0
    if Cin % 64 == 0 and KH * KW <= 32:
        return 1
    if not is1x1 and KH <= 32 and cdiv(KW * Cin, 64) <= 32 and KW * Cin >= 48:
        return 2
    return 0


def split_count(M, Cout, K):
    """Slices along K of a few-tile, deep-K problem (before the 'no empty slice' re-division)."""
    if Cout % 8:
        return 1
    tiles, nk = cdiv(M, 64) * cdiv(Cout, 64), cdiv(K, 64)
    if tiles >= 192 or nk < 24:
        return 1
    s = min(cdiv(448, tiles), nk // 4)
    return max(1, min(s, 16))


def _grid(M, Cout, tile, xcd_ok=True):
    """(xcd_ny, grid) of an unsplit launch: the XCD-aware 1-D order needs more than one column tile and >= 16 row tiles."""
    gx, gy = cdiv(M, tile), cdiv(Cout, tile)
    if xcd_ok and gy > 1 and gx >= 16:
        return gy, (8 * cdiv(gx, 8) * gy, 1, 1)
    return 0, (gx, gy, 1)


def _plan(family, tile, ring, is1x1, fast, splits, steps, xcd_ny, grid, threads=256):
    return dict(zip(FIELDS, (family, tile, ring, int(is1x1), fast, splits, steps, xcd_ny, *grid, threads)))


def plan(H, W, Cin, Cout, k=1, stride=1, pad=0, batch=1, has_ws=False, entry=CONV2D, extra=0, pc=2, ldx=0):
    """extra: Cin2 of the dual form, n of the grouped one.  pc: the RMEM_GEMM_PC setting (2 when unset)."""
    Ho, Wo = out_size(H, W, k, stride, pad)
    M, K = batch * Ho * Wo, k * k * Cin
    is1x1 = k == 1 and stride == 1 and pad == 0
    fast = fast_form(H, W, Cin, Cout, k, k, stride, pad, batch, ldx)
    t128 = cdiv(M, 128) * cdiv(Cout, 128)
    if entry == DUAL:
        K = Cin + extra
        if Cout >= 128 and K >= 256 and t128 >= 128:
            xcd, grid = _grid(M, Cout, 128)
            return _plan(DUAL128, 128, 1, True, fast, 1, K // 64, xcd, grid)
        xcd, grid = _grid(M, Cout, 64)
        return _plan(DUAL64, 64, 1, True, fast, 1, K // 64, xcd, grid)
    nk = cdiv(K, 64)
    if entry == LINEAR_GROUPED:
        gx, gy = cdiv(M, 64), cdiv(Cout, 64)
        ring = 3 if fast == 1 and gx * gy * extra <= 1024 and nk >= 3 else 1
        return _plan(GROUPED, 64, ring, True, fast, 1, nk, 0, (gx, gy, extra))
    splits, steps = (split_count(M, Cout, K) if has_ws else 1), nk
    if splits > 1:
        steps = cdiv(nk, splits)
        splits = cdiv(nk, steps)
        return _plan(GENERAL64, 64, 1, is1x1, fast, splits, steps, 0, (cdiv(M, 64), cdiv(Cout, 64), splits))
    if fast == 1 and Cout >= 128 and K >= 512 and t128 >= 128:
        xcd, grid = _grid(M, Cout, 128)
        deep = 3 if t128 <= 256 else 1          # what the one-role kernel would take
        ring = {0: deep, 1: 3 if deep == 3 else 2, 2: 2, 3: 3}[pc]
        return _plan(ONE128 if pc == 0 else PC128, 128, ring, is1x1, fast, 1, steps, xcd, grid, 256 if pc == 0 else 512)
    if fast == 2 and Cout >= 128:
        xcd, grid = _grid(M, Cout, 128)
        return _plan(ROWRUN128, 128, 3, False, fast, 1, steps, xcd, grid)
    xcd, grid = _grid(M, Cout, 64)
    ring = 3 if fast and cdiv(M, 64) * cdiv(Cout, 64) <= 1024 and steps >= 3 else 1
    return _plan((GENERAL64, SCALAR64, ROWRUN64)[fast], 64, ring, is1x1, fast, 1, steps, xcd, grid)


def kernels(p):
    """The kernel instantiations a plan launches: (family, ring, is1x1) plus what else selects a template argument -- the split-K
    form of the general kernel (and its epilogue kernel), the fast / general form of the grouped one."""
    if p['family'] == GENERAL64 and p['splits'] > 1:
        return {('general64', 1, p['is1x1'], 'split'), ('splitk_epilogue',)}
    if p['family'] == GROUPED:
        return {('grouped', p['ring'], 1, 'fast' if p['fast'] == 1 else 'general')}
    return {(FAMILY_NAMES[p['family']], p['ring'], p['is1x1'])}


# every instantiation gemm_conv.hip builds, per element type
ALL_KERNELS = (
    {('general64', 1, i) for i in (0, 1)} | {('general64', 1, i, 'split') for i in (0, 1)} | {('splitk_epilogue',)}
    | {('scalar64', r, i) for r in (1, 3) for i in (0, 1)} | {('rowrun64', r, 0) for r in (1, 3)}
    | {('one128', r, i) for r in (1, 3) for i in (0, 1)} | {('pc128', r, i) for r in (2, 3) for i in (0, 1)}
    | {('rowrun128', 3, 0), ('dual64', 1, 1), ('dual128', 1, 1)}
    | {('grouped', 3, 1, 'fast'), ('grouped', 1, 1, 'fast'), ('grouped', 1, 1, 'general')})
assert len(ALL_KERNELS) == 25
