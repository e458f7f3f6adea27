"""CPU checks of tests/gated_ref.py, the yardstick of the gated-attention GPU tests in tests/test_hip_deaot_ops.py:
the float64 references agree with the oracle (oracle/deaot_cpu.py, fp32), every GPU case reaches the launch plan it was chosen for,
and every GPU case's inputs expose the bugs the case exists for: a mutated reference moves by more than 5x the tolerance the GPU test
applies, in the GPU test's own metric (max |difference| over max |reference| of the clip; absolute for the mass)."""
import pytest
import torch

import gated_ref as G
from gated_ref import DV, KT, LOCAL_CASES, LONG_CASES, MASS_TOL, SELF_CASES, TOL
from oracle import deaot_cpu as D
from rmem_ocu_amd.runtime import temporal_slots
from test_hip_ops import seeded

BF16, F16 = torch.bfloat16, torch.float16
DTS = [BF16, F16]


def identity_tail(p):
    """Weights that turn the oracle's dw_conv + projection into the identity, so its modules return `attention * U` itself."""
    dw = torch.zeros(DV, 1, 5, 5)
    dw[:, 0, 2, 2] = 1
    return {p + '.dw_conv.conv.weight': dw, p + '.projection.weight': torch.eye(DV), p + '.projection.bias': torch.zeros(DV)}


def rel_err(got, ref):
    return ((got.double() - ref.double()).abs().max() / ref.abs().max()).item()


# ------------------------------------------------------------------ references vs the oracle
@pytest.mark.parametrize('h,wd', [(9, 11), (18, 23)])
def test_gated_ref_matches_oracle(h, wd):
    T, L = 3, h * wd
    q, k = seeded(901, (L, 128), 1.5), seeded(902, (T, L, 128), 1.5)
    v, u = seeded(903, (T, L, DV)), seeded(904, (L, DV))
    pe_cur, pe_mem, slots = seeded(905, (128,), 0.5), seeded(906, (4, 128), 0.5), [2, 0, 3]
    ref, mass = G.gated_ref(q, k, v, u, pe_cur, pe_mem, slots)
    K = (k + pe_mem[slots][:, None, :]).reshape(T * L, 1, 128)
    out, attn = D.gated_propagation((q + pe_cur).view(L, 1, 128), K, v.reshape(T * L, 1, DV), u.view(L, 1, DV), (h, wd),
                                    identity_tail('m'), 'm', use_linear=False, explicit=True)
    assert rel_err(out[:, 0], ref) < 1e-5
    assert (attn[0, 0].view(L, T, L).sum(2).double() - mass).abs().max().item() < 1e-5
    assert (mass.sum(1) - 1).abs().max().item() < 1e-12
    # the layer-0 gate: a narrower u is [u | ones]
    half, _ = G.gated_ref(q, k, v, u[:, :512], pe_cur, pe_mem, slots)
    ones, _ = G.gated_ref(q, k, v, torch.cat([u[:, :512], torch.ones(L, 512)], 1), pe_cur, pe_mem, slots)
    assert torch.equal(half, ones)


@pytest.mark.parametrize('h,wd', [(9, 11), (18, 23)])
def test_local_gated_ref_matches_oracle(h, wd):
    L = h * wd
    q2, k2 = seeded(911, (1, 128, h, wd), 1.5), seeded(912, (1, 128, h, wd), 1.5)
    v2, u = seeded(913, (1, DV, h, wd)), seeded(914, (L, 1, DV))
    w = identity_tail('m')
    w['m.relative_emb_k.weight'], w['m.relative_emb_k.bias'] = seeded(915, (225, 128, 1, 1), 0.1), seeded(916, (225,), 0.5)
    out = D.local_gated_propagation(q2, k2, v2, u, (h, wd), w, 'm')
    tok = lambda x: x[0].permute(1, 2, 0).reshape(L, -1)      # noqa: E731
    q = tok(q2)
    rel = q.double() @ w['m.relative_emb_k.weight'].view(225, 128).double().t() + w['m.relative_emb_k.bias'].double()
    ref = G.local_gated_ref(q, tok(k2), tok(v2), rel, u[:, 0], h, wd)
    assert rel_err(out[:, 0], ref) < 1e-5


def test_dwconv5x5_ref_matches_oracle():
    h, wd, C = 9, 11, 64
    x, w = seeded(921, (h * wd, C)), seeded(922, (25, C), 0.2)
    out = D.dw_conv(x.view(h * wd, 1, C), (h, wd), w.t().reshape(C, 1, 5, 5))
    assert rel_err(out[:, 0], G.dwconv5x5_ref(x, w, h, wd)) < 1e-5


# ------------------------------------------------------------------ every GPU case reaches the plan it was chosen for
@pytest.mark.parametrize('case', LONG_CASES, ids=lambda c: c.name)
def test_long_case_plan(case):
    L = case.H * case.W
    rows = G.frame_rows(case.T, L, case.splits)
    p = G.table_plan(L, rows, case.T, L, case.clips)
    assert (p.groups, p.key_tiles, p.empty_groups) == (case.groups, case.key_tiles, case.empty)
    assert p.nrows == case.T * case.splits <= 64
    if case.name == 'mid-row-ranges':
        assert [r[2] for r in rows[:2]] == [192, 108] and temporal_slots(case.T) != list(range(case.T))
        row_starts, n = set(), 0
        for r in rows:
            row_starts.add(n)
            n += -(-r[2] // KT)
        assert any(g * p.tiles_per_group not in row_starts for g in range(1, p.groups)), 'a key group begins inside a table row'
    # one clip of the same shape (what every earlier op test launched) takes another plan
    assert G.table_plan(L, rows, case.T, L, 1).groups != case.groups or case.name == 'empty-groups'


def test_bench_geometry_plan():
    """8 clips of 31 x 54 tokens: one key group, 4 local and self-attention ranges (group_runtime_deaot.py's rule is the same)."""
    L = 31 * 54
    assert G.plan_groups(L, 9, L, 8) == 1 and G.local_ranges(L, 8) == 4 and G.local_ranges(L, 1) == 8


@pytest.mark.parametrize('case', SELF_CASES, ids=lambda c: c.name)
def test_self_case_plan(case):
    p = G.range_plan(case.H * case.W, case.nchunks, case.clips)
    assert (p.nrows, p.groups) == (case.nrows, case.groups)
    if case.name == 'one-group':
        assert p.per == 128 and case.H * case.W - p.per == 15


@pytest.mark.parametrize('case', LOCAL_CASES, ids=lambda c: c.name)
def test_local_case_plan(case):
    L = case.H * case.W
    p = G.local_plan(L, case.clips)
    assert (p.nrows, p.groups) == (case.nrows, case.groups)
    if case.name == '2-ranges':
        assert G.local_ranges(L, case.clips - 1) == 3, 'the smallest clip count with 2 ranges'
    if (case.H, case.W) == (18, 23):
        assert G.band_tiles(18, 23, 0) == (0, 5) and p.key_tiles == 7        # band skipping: 5 of 7 key tiles


# ------------------------------------------------------------------ the cases' inputs can see the bugs
def moved(mut, ref, tol):
    """How far a mutated reference is from the true one, in units of the GPU test's tolerance."""
    return rel_err(mut, ref) / tol


def tile_masks(T, L):
    """keep masks [T, L]: keys 64..127 of frame T // 2 dropped; the last, partial tile of the last frame dropped."""
    assert L % KT, 'the cases end in a partial tile'
    one, last = torch.ones(T, L, dtype=torch.bool), torch.ones(T, L, dtype=torch.bool)
    one[T // 2, KT:2 * KT] = False
    last[T - 1, L // KT * KT:] = False
    return one, last


def check_long(x, c, slots, ub, tol):
    """x: inputs with a clip dimension (>= 2 clips), c: the clip under test."""
    T, L = x['k'].shape[1:3]
    args = (x['q'][c], x['k'][c], x['v'][c])
    u = x['u'][c] if ub else x['u'][c][:, :512]
    pe = (x['pe_cur'], x['pe_mem'])
    ref, mass = G.gated_ref(*args, u, *pe, slots)
    for keep in tile_masks(T, L):
        assert moved(G.gated_ref(*args, u, *pe, slots, keep=keep)[0], ref, tol) > 5
    if T > 1:
        a, b = 0, next(t for t in range(T - 1, 0, -1) if slots[t] != slots[0])
        swapped = list(slots)
        swapped[a], swapped[b] = slots[b], slots[a]
        assert moved(G.gated_ref(*args, u, *pe, swapped)[0], ref, tol) > 5
        perm = list(range(T))
        perm[0], perm[1] = 1, 0
        assert (mass[:, perm] - mass).abs().max().item() > 5 * MASS_TOL
    other = x['u'][c][:, :512] if ub else x['u'][c]
    assert moved(G.gated_ref(*args, other, *pe, slots)[0], ref, tol) > 5
    if x['q'].shape[0] > 1:
        nxt = G.gated_ref(x['q'][c + 1], x['k'][c + 1], x['v'][c + 1], x['u'][c + 1] if ub else x['u'][c + 1][:, :512], *pe, slots)
        assert moved(nxt[0], ref, tol) > 5 and (nxt[1] - mass).abs().max().item() > 5 * MASS_TOL


@pytest.mark.parametrize('dt', DTS, ids=str)
@pytest.mark.parametrize('case', LONG_CASES, ids=lambda c: c.name)
def test_long_case_inputs_see_mutations(case, dt):
    check_long(G.long_inputs(case, dt, clips=2), 0, temporal_slots(case.T), case.ub, TOL[dt])


@pytest.mark.parametrize('T,L', [(1, 99), (3, 200)])
def test_temporal_pe_f16_inputs_see_mutations(T, L):
    x = G.temporal_pe_inputs(T, L, F16)
    check_long({k: (v if k.startswith('pe') else v[None]) for k, v in x.items()}, 0, temporal_slots(T), True, TOL[F16])


@pytest.mark.parametrize('dt', DTS, ids=str)
@pytest.mark.parametrize('case', SELF_CASES, ids=lambda c: c.name)
def test_self_case_inputs_see_mutations(case, dt):
    L, tol = case.H * case.W, TOL[dt]
    x = G.self_inputs(case, dt, clips=2)
    parts = lambda c: (x[c, :, :128], x[c, :, :128][None], x[c, :, 128:128 + DV][None], x[c, :, 128 + DV:])      # noqa: E731
    q, k, v, u = parts(0)
    ref, _ = G.gated_ref(q, k, v, u)
    for keep in tile_masks(1, L):
        assert moved(G.gated_ref(q, k, v, u, keep=keep)[0], ref, tol) > 5
    assert moved(G.gated_ref(q, k, v, u[:, :512])[0], ref, tol) > 5
    assert moved(G.gated_ref(*parts(1))[0], ref, tol) > 5


@pytest.mark.parametrize('dt', DTS, ids=str)
@pytest.mark.parametrize('case', LOCAL_CASES, ids=lambda c: c.name)
def test_local_case_inputs_see_mutations(case, dt):
    H, W, tol = case.H, case.W, TOL[dt]
    x = G.local_inputs(case, dt, clips=2)
    gate = lambda c, ub: x['u'][c] if ub else x['u'][c][:, :512]      # noqa: E731
    args = (x['q'][0], x['k'][0], x['v'][0], x['rel'][0])
    ref = G.local_gated_ref(*args, gate(0, case.ub), H, W)
    for keep in tile_masks(1, H * W):
        assert moved(G.local_gated_ref(*args, gate(0, case.ub), H, W, keep=keep[0]), ref, tol) > 5
    assert moved(G.local_gated_ref(*args, gate(0, case.ub), H, W, dx_shift=1), ref, tol) > 5
    assert moved(G.local_gated_ref(*args, gate(0, case.ub), H, W, radius=6), ref, tol) > 5
    assert moved(G.local_gated_ref(*args, gate(0, not case.ub), H, W), ref, tol) > 5
    nxt = G.local_gated_ref(x['q'][1], x['k'][1], x['v'][1], x['rel'][1], gate(1, case.ub), H, W)
    assert moved(nxt, ref, tol) > 5
    # the relative embedding of the next clip (the rel clip stride), everything else of this clip
    assert moved(G.local_gated_ref(x['q'][0], x['k'][0], x['v'][0], x['rel'][1], gate(0, case.ub), H, W), ref, tol) > 5
