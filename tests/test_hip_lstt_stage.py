"""The GroupRuntime stage programs (prog_lstt propagate and reference mode, prog_update, prog_project, prog_decode) against the
float64 oracle of tests/lstt_ref.py, from seeded buffers of unit scale: which buffer feeds which op, where rounding happens, the
per-clip chunk tables and how dec_in is assembled.  The bit-identity tests (tests/test_hip_chain_blocks.py,
test_lstt_chains_are_bit_identical) pin the routes to each other; these pin every route to the maths.

Per tensor: emax = max |got - ref| / max |ref|, erms = rms(got - ref) / rms(ref), judged by lstt_ref.tolerances (3x / 2x the distance
rounding alone moves the reference, measured on the CPU on each case's own inputs; tests/test_lstt_ref_host.py holds them under a third of every mutation).

Measured on MI355X, worst tensor over all cases and routes of a stage, as a fraction of its tolerance and in absolute terms:
  stage (cases)                          type   emax <=   erms <=   worst emax / T   worst erms / T
  prog_lstt propagate (44 cases)         bf16   8.5e-3    6.3e-3    0.60 (mass)      0.64 (tgt3 column means)
                                         fp16   9.5e-4    8.0e-4    0.56 (mass)      0.60 (mass)
      of which the mass                  bf16   2.2e-3    7.2e-4
                                         fp16   2.5e-4    8.9e-5
  prog_lstt reference frame (2 sizes)    bf16   7.5e-3    6.1e-3    0.47 (h1)        0.57 (tgt3 column means)
                                         fp16   9.4e-4    7.7e-4    0.46             0.56
  prog_update (append off / on)          bf16   3.7e-3    2.5e-3    0.33 (short_V)   0.50 (short_K)
                                         fp16   4.8e-4    3.1e-4    0.33             0.50
  prog_project, dec_in[:, :256]          bf16   2.6e-3    1.7e-3    0.33             0.50
                                         fp16   3.3e-4    2.1e-4    0.33             0.50
      fp32 x (tolerance 6.1e-5)          both   4.4e-7    2.0e-7
  prog_decode (3 sizes x 4 routes)       bf16   5.5e-3    3.5e-3    0.42 (logits)    0.60 (logits)
                                         fp16   7.6e-4    4.4e-4    0.45             0.61
The unfused list and the chains give the same figures (they are bit-identical); 0.50 of an erms tolerance is the rounding distance
itself (T = 2 * d_round): the GPU sits where the emulated rounding puts it, and what it adds (softmax weights in 16 bits, fp32
accumulation order, split-K) is inside the margin.
"""
import pytest
import torch

import lstt_ref as R
from test_hip_chain_blocks import env, packed

pytestmark = pytest.mark.gpu
F64 = torch.float64
C, NL = 256, 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def runtime(dev, dt, hw, S, B, align=True):
    from rmem_ocu_amd.group_runtime import GroupRuntime
    return GroupRuntime(packed(dt), hw, S, dev, B, align_corners=align, lookahead=1)


def stream():
    return torch.cuda.current_stream().cuda_stream


def judge(stage, dt, case, got, ref, tol, keys):
    """Every compared tensor within its tolerance in both metrics; prints each figure before it asserts."""
    bad = []
    for k in keys:
        assert torch.isfinite(got[k].float()).all(), (case, k)
        emax, erms = R.metrics(got[k], ref[k])
        print(f'MEASURED {stage} {dt} {case} {k} emax {emax:.3e} erms {erms:.3e} T {tol[k][0]:.3e} {tol[k][1]:.3e}')
        if not (emax <= tol[k][0] and erms <= tol[k][1]):
            bad.append((k, f'emax {emax:.3e} > {tol[k][0]:.3e}' if emax > tol[k][0] else f'erms {erms:.3e} > {tol[k][1]:.3e}'))
    assert not bad, (stage, dt, case, bad)


def sentinel(t, seed):
    """Fill a 16-bit buffer with a seeded pattern of finite values and return a copy to compare with, bit for bit."""
    t.copy_(R.seeded(seed, tuple(t.shape), 3.0))
    return t.clone()


# ------------------------------------------------------------------ prog_lstt, propagate
def run_propagate(dev, dt, hw, slots, S, route):
    from rmem_ocu_amd import ops
    B = len(slots)
    rt = runtime(dev, dt, hw, S, B)
    rt.chain = route != 'unfused'
    rt.merge_fold = route != 'nofold'
    R.fill_lstt_state(rt)
    rt.slots = [list(s) for s in slots]
    T, L = rt.T, rt.L
    rt.mass.fill_(-1.0)
    s = stream()
    rt.prepare_pos(s)
    rt.upload_chunks(s)
    with env(RMEM_CHAIN_ROWS=64 if route == 'rows64' else None):
        prog = rt.prog_lstt(False, T, True)
        ops.run(prog, s)
        torch.cuda.synchronize()
    chains = sum(op.name.startswith('rmem_lstt_chain') for op in prog)
    assert (len(prog), chains) == ((48, 0) if route == 'unfused' else (19, 10)), (route, len(prog), chains)
    got = {'x2': rt.x, 'k4_2': rt.k4, 'v4_2': rt.v4, 'h1_2': rt.h1, 'h3_2': rt.h3, 'mass': rt.mass[:B * L * T].view(B, L, T)}
    for i in range(NL):
        got.update({f'cq{i}': rt.curr_Q[i], f'cv{i}': rt.curr_V[i], f'tgt3_{i}': rt.tgt3[i], f'dec{i}': rt.dec_in[:, (i + 1) * C:(i + 2) * C]})
    return R.with_column_means({k: v.detach().to('cpu', F64) for k, v in got.items()})


def check_propagate(dev, dt, case, route):
    hw, S, slots = R.LSTT_CASES[case]
    ref = R.reference_case('lstt', dt, case)
    got = run_propagate(dev, dt, hw, slots, S, route)
    judge('lstt', dt, f'{case}/{route}', got, ref, R.tolerances('lstt', dt, case=case), R.lstt_compared())
    m = got['mass']
    assert (m.sum(-1) - 1).abs().max().item() < 1e-4
    for c, s in enumerate(slots):
        assert (m[c, :, len(s):] == 0).all(), f'clip {c}: mass on frames its bank does not have'
        assert (m[c, :, :len(s)] > 0).all()


SIZES = {(161, 193): 143, (129, 257): 153}


@pytest.mark.parametrize('route', ['unfused', 'chained'])
@pytest.mark.parametrize('T', [1, 2, 5, 8])
@pytest.mark.parametrize('hw', sorted(SIZES))
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_lstt_propagate_against_the_oracle(dev, dt, hw, T, route):
    """Three clips through the three blocks against lstt_block / ln in float64: 143 tokens (four 32-row blocks + one of 15 rows) and
    153; T = 1, 2 (four key ranges per frame), 5 and 8 (flip / nearest temporal slots, one range per frame); bank slots shuffled
    per clip; the unfused launch list and the row chains."""
    case = f'{SIZES[hw]}tok/T{T}'
    assert R.LSTT_CASES[case][0] == hw and all(len(s) == T for s in R.LSTT_CASES[case][2])
    check_propagate(dev, dt, case, route)


@pytest.mark.parametrize('route', ['rows64', 'nofold'])
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_lstt_propagate_chain_variants_against_the_oracle(dev, dt, route):
    """143 tokens, T = 2: 64-row chain blocks (RMEM_CHAIN_ROWS=64) and the merge pass instead of the folded merge."""
    check_propagate(dev, dt, '143tok/T2', route)


@pytest.mark.parametrize('route', ['unfused', 'chained'])
@pytest.mark.parametrize('case', ['banks-2-1-2', 'banks-1-5-2'])
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_lstt_propagate_unequal_banks_against_the_oracle(dev, dt, case, route):
    """Clips with banks of different length in one group: the reference runs each clip alone with its own T (its own temporal
    slots, its own softmax), which is what the padded chunk table claims to reproduce; padded frames carry exactly zero mass."""
    assert [len(s) for s in R.LSTT_CASES[case][2]] == [int(n) for n in case.split('-')[1:]]
    check_propagate(dev, dt, case, route)


# ------------------------------------------------------------------ prog_lstt, reference frame
@pytest.mark.parametrize('hw', sorted(SIZES))
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_lstt_reference_frame_against_the_oracle(dev, dt, hw):
    """prog_lstt(ref_mode=True) from seeded x and id_emb against lstt_block with curr_id_emb: the block outputs, the bank entry
    scattered to the slots of upload_append_slots, short_K / short_V; every other bank slot keeps its sentinel bit for bit."""
    from rmem_ocu_amd import ops
    B, S, dest = 3, 4, [2, 0, 3]
    case = f'{SIZES[hw]}tok'
    assert R.CASES['lstt_ref'][case] == hw and B == R.CLIPS
    _, _, size, st, _, _, ide = R.stage_args('lstt_ref', dt, case)
    L = size[0] * size[1]
    ref = R.reference_case('lstt_ref', dt, case)
    rt = runtime(dev, dt, hw, S, B)
    rt.x.copy_(st['x']); rt.id_emb.copy_(ide)
    before = {}
    for i in range(NL):
        before[f'K{i}'], before[f'V{i}'] = sentinel(rt.bank_K[i], 500 + i), sentinel(rt.bank_V[i], 510 + i)
        sentinel(rt.short_K[i], 520 + i); sentinel(rt.short_V[i], 530 + i)
    rt.slots = [[d] for d in dest]
    s = stream()
    rt.prepare_pos(s)
    rt.upload_chunks(s)
    rt.upload_append_slots(dest, s)
    ops.run(rt.prog_lstt(True, 1), s)
    torch.cuda.synchronize()
    rows = [c * S + d for c, d in enumerate(dest)]
    others = [r for r in range(B * S) if r not in rows]
    got = {'x2': rt.x, 'k4_2': rt.k4, 'v4_2': rt.v4, 'h1_2': rt.h1, 'h3_2': rt.h3}
    for i in range(NL):
        got.update({f'cq{i}': rt.curr_Q[i], f'cv{i}': rt.curr_V[i], f'tgt3_{i}': rt.tgt3[i], f'dec{i}': rt.dec_in[:, (i + 1) * C:(i + 2) * C],
                    f'bank_K{i}': rt.bank_K[i][rows].reshape(B * L, C), f'bank_V{i}': rt.bank_V[i][rows].reshape(B * L, C),
                    f'short_K{i}': rt.short_K[i], f'short_V{i}': rt.short_V[i]})
        assert torch.equal(rt.bank_K[i][others], before[f'K{i}'][others]) and torch.equal(rt.bank_V[i][others], before[f'V{i}'][others]), i
        assert torch.equal(rt.bank_K[i][rows].reshape(B * L, C), rt.curr_Q[i]) and torch.equal(rt.bank_V[i][rows].reshape(B * L, C), rt.new_V[i])
    got = R.with_column_means({k: v.detach().to('cpu', F64) for k, v in got.items()})
    judge('lstt_ref', dt, case, got, ref, R.tolerances('lstt_ref', dt, case=case), R.lstt_compared(True))


# ------------------------------------------------------------------ prog_update
@pytest.mark.parametrize('append', [False, True])
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_update_against_the_oracle(dev, dt, append):
    """prog_update from seeded tgt3 / curr_V / curr_Q / id_emb against OracleEngine._update_memories: short_K, short_V, and with
    append new_V and the entries scattered into the banks; clip 1's destination slot is -1, so nothing of its bank changes, and
    nothing changes in any other slot."""
    from rmem_ocu_amd import ops
    B, S, case, dest = R.CLIPS, 4, '143tok', [2, -1, 0]
    rt = runtime(dev, dt, R.CASES['update'][case], S, B)
    _, st, _, L = R.stage_args('update', dt, case)
    assert L == rt.L
    ref = R.reference_case('update', dt, case)
    rt.id_emb.copy_(st['id_emb'])
    before = {}
    for i in range(NL):
        rt.tgt3[i].copy_(st['tgt3'][i]); rt.curr_V[i].copy_(st['curr_V'][i]); rt.curr_Q[i].copy_(st['curr_Q'][i])
        before[f'K{i}'], before[f'V{i}'] = sentinel(rt.bank_K[i], 600 + i), sentinel(rt.bank_V[i], 610 + i)
        before[f'N{i}'] = sentinel(rt.new_V[i], 620 + i)
        sentinel(rt.short_K[i], 630 + i); sentinel(rt.short_V[i], 640 + i)
    s = stream()
    rt.upload_append_slots(dest, s)
    ops.run(rt.prog_update(append), s)
    torch.cuda.synchronize()
    written = {c * S + d: c for c, d in enumerate(dest) if d >= 0} if append else {}
    others = [r for r in range(B * S) if r not in written]
    got, keys = {}, []
    for i in range(NL):
        got.update({f'short_K{i}': rt.short_K[i], f'short_V{i}': rt.short_V[i]})
        keys += [f'short_K{i}', f'short_V{i}']
        assert torch.equal(rt.bank_K[i][others], before[f'K{i}'][others]) and torch.equal(rt.bank_V[i][others], before[f'V{i}'][others]), i
        if append:
            got[f'new_V{i}'] = rt.new_V[i]
            keys.append(f'new_V{i}')
            for r, c in written.items():
                assert torch.equal(rt.bank_K[i][r], rt.curr_Q[i][c * L:(c + 1) * L]), (i, r)
                assert torch.equal(rt.bank_V[i][r], rt.new_V[i][c * L:(c + 1) * L]), (i, r)
                em, er = R.metrics(rt.bank_K[i][r], ref[f'bank_K{i}'][c * L:(c + 1) * L])
                assert em == 0 and er == 0
        else:
            assert torch.equal(rt.new_V[i], before[f'N{i}'])
    judge('update', dt, f'append{int(append)}', got, ref, R.tolerances('update', dt, case=case), keys)


# ------------------------------------------------------------------ prog_project
@pytest.mark.parametrize('hw', sorted(SIZES))
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_project_against_the_oracle(dev, dt, hw):
    """prog_project(None) from a seeded encoder output: the fp32 residual stream and its 16-bit copy in dec_in[:, :256]; columns 256
    onward keep their sentinel."""
    from rmem_ocu_amd import ops
    B, case = R.CLIPS, f'{SIZES[hw]}tok'
    assert R.CASES['project'][case] == hw
    rt = runtime(dev, dt, hw, 4, B)
    enc3 = R.stage_args('project', dt, case)[1]
    ref = R.reference_case('project', dt, case)
    rt.enc_now.enc_out[2].view(B * rt.L, 1024).copy_(enc3)
    before = sentinel(rt.dec_in, 700)
    rt.x.fill_(float('nan'))
    ops.run(rt.prog_project(None), stream())
    torch.cuda.synchronize()
    assert torch.equal(rt.dec_in[:, C:], before[:, C:])
    judge('project', dt, case, {'x': rt.x, 'dec0': rt.dec_in[:, :C]}, ref, R.tolerances('project', dt, case=case), ['x', 'dec0'])


# ------------------------------------------------------------------ prog_decode
@pytest.mark.parametrize('route', sorted(R.DECODE_ROUTES))
@pytest.mark.parametrize('case', sorted(R.CASES['decode']))
@pytest.mark.parametrize('dt', ['bf16', 'fp16'])
def test_decode_against_the_oracle(dev, dt, case, route):
    """prog_decode(None) from seeded encoder outputs and dec_in against fpn_decode: logits[:, :11] and the stage outputs d16a, d8d,
    d4a, two images, with and without align_corners, on the default route and the three switches (read when the program is built:
    a fresh runtime per setting, the environment restored after)."""
    from rmem_ocu_amd import ops
    _, enc, dec_in, B, hw, align = R.stage_args('decode', dt, case)
    assert (case, align) in (('161x193', True), ('129x257', True), ('160x192', False))
    ref = R.reference_case('decode', dt, case)
    with env(**{k: R.DECODE_ENV[route].get(k) for k in ('RMEM_NO_UPFUSE', 'RMEM_DIRECT_CONV3_128', 'RMEM_NO_HEADFUSE')}):
        rt = runtime(dev, dt, hw, 4, B, align)
        prog = rt.prog_decode(None)
    names = [op.name for op in prog]
    assert ('rmem_conv3x3_direct' in names) == (route == 'direct128'), names
    assert len(prog) == {'default': 11, 'direct128': 11, 'no_upfuse': 13, 'no_headfuse': 12}[route], names
    for buf, t in zip(rt.enc_now.enc_out, enc):
        buf.view(t.shape).copy_(t)
    rt.dec_in.copy_(dec_in)
    rt.logits.fill_(float('nan'))
    ops.run(prog, stream())
    torch.cuda.synchronize()
    got = {'logits': rt.logits[:, :11], 'd16a': rt.d16a, 'd8d': rt.d8b.view(-1)[:B * rt.M8 * 128].view(B * rt.M8, 128), 'd4a': rt.d4a}
    judge('decode', dt, f'{case}/{route}', got, ref, R.tolerances('decode', dt, R.DECODE_ROUTES[route], case), ['logits', 'd16a', 'd8d', 'd4a'])
