"""The stage references of tests/lstt_ref.py, checked on the CPU: the op-by-op restatement IS the oracle (1e-12), every wrong
reference of the mutation lists is further than 3 * T from the right one, and no tolerance of any GPU case is wider than the caps
of test_case_tolerances_stay_under_the_caps.  To see that the tests have teeth, make ``reference_of`` below return a wrong reference
(``R._canon(stage, dt)[2](R.MUTATIONS[stage][-1])``, or any other entry) and watch test_restatement_is_the_oracle fail."""
import os

import pytest
import torch

import lstt_ref as R

DTS = ('bf16', 'fp16')


def reference_of(stage, dt):
    return R._canon(stage, dt)[0]


def compared(stage):
    return R.lstt_compared(stage == 'lstt_ref') if stage.startswith('lstt') else sorted(R.tolerances(stage, 'bf16'))


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('stage', R.STAGES)
def test_restatement_is_the_oracle(stage, dt):
    """With rounding switched off the restatement equals oracle.ref_cpu (lstt_block + ln, _update_memories, the projector's conv,
    fpn_decode) in float64 to 1e-12 of each tensor, on every output the references return: banks of 1, 5 and 2 frames in shuffled
    slots for the propagate stage."""
    ref, plain = reference_of(stage, dt), R._canon(stage, dt)[2](None)
    assert set(ref) == set(plain)
    for k in ref:
        emax, erms = R.metrics(plain[k], ref[k])
        assert emax < 1e-12 and erms < 1e-12, (stage, k, emax, erms)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('stage', R.STAGES)
def test_every_mutation_is_further_than_three_tolerances(stage, dt):
    """Every wrong reference moves at least one tensor the GPU tests compare by more than 3 * T in emax AND in erms, T being that
    tensor's tolerance.  Prints d_round and the mutation distances."""
    tol, dr, dist = R.tolerances(stage, dt), R.d_round(stage, dt), R.mutation_distances(stage, dt)
    keys = compared(stage)
    print(f'\n{stage} {dt}: d_round (emax, erms) and T per compared tensor')
    for k in keys:
        print(f'  {k:10s} d_round {dr[k][0]:.2e} {dr[k][1]:.2e}   T {tol[k][0]:.2e} {tol[k][1]:.2e}')
    assert len(dist) == len(R.MUTATIONS[stage]) >= 3
    for m, d in dist.items():
        k = witness(d, tol, keys)
        ra, rb = d[k][0] / tol[k][0], d[k][1] / tol[k][1]
        print(f'  {m:36s} on {k:9s} emax {d[k][0]:.2e} = {ra:7.1f} T   erms {d[k][1]:.2e} = {rb:7.1f} T')
        assert ra > 3 and rb > 3, (stage, dt, m, k, d[k], tol[k])


def witness(d, tol, keys):
    """The compared tensor on which a mutation shows most, in units of the tolerance (the smaller of the two metrics' ratios)."""
    return max(keys, key=lambda k: min(d[k][0] / tol[k][0], d[k][1] / tol[k][1]))


ALL_CASES = [(stage, case) for stage in R.STAGES for case in sorted(R.CASES[stage])]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('stage,case', ALL_CASES)
def test_case_tolerances_stay_under_the_caps(stage, case, dt):
    """Every case of the GPU tests is judged by tolerances measured on its own inputs; each of them (the decoder's also with the
    unfused routes' extra rounding points) must meet two conditions, whatever it was derived from.

    The independent one: no tolerance is wider than 16 (emax) / 8 (erms) units of the element type's rounding, 2^-9 bf16 and 2^-11
    fp16 relative.  Three blocks of about ten store points, each at most unit / sqrt(3) rms, add in quadrature to 3.2 units;
    times the margins 3 and 2 that is 9.6 and 6.4.  This holds for every compared tensor, also those no listed mutation needs.

    The other, T <= a third of the mutation distance, can only be asked on a mutation's witness tensor (a mutation that does not
    touch a tensor has distance 0 there).  For the canonical case that is the inequality of
    test_every_mutation_is_further_than_three_tolerances restated; what it adds is the other cases, whose own tolerances are held
    against the distances measured on the canonical one."""
    for route in (sorted(set(R.DECODE_ROUTES.values())) if stage == 'decode' else [()]):
        tol = R.tolerances(stage, dt, route, case)
        if route == ():
            print(f'\n{stage} {case} {dt}: ' + '  '.join(f'{k} {a:.1e}/{b:.1e}' for k, (a, b) in tol.items() if k in SHOWN))
        check_cap(stage, dt, tol)


SHOWN = ('x2', 'tgt3_2', 'tgt3m_2', 'mass', 'short_K2', 'new_V2', 'x', 'dec0', 'logits', 'd8d')


def check_cap(stage, dt, tol):
    dist, keys = R.mutation_distances(stage, dt), compared(stage)
    unit = {'bf16': 2.0 ** -9, 'fp16': 2.0 ** -11}[dt]
    for k in keys:
        assert tol[k][0] <= 16 * unit and tol[k][1] <= 8 * unit, (stage, dt, k, tol[k])
    for m, d in dist.items():
        k = witness(d, tol, keys)
        assert tol[k][0] <= d[k][0] / 3 and tol[k][1] <= d[k][1] / 3, (stage, dt, m, k, tol[k], d[k])


def test_gpu_cases_are_the_cases_measured_here():
    """tests/test_hip_lstt_stage.py takes inputs, references and tolerances of every case from lstt_ref (stage_args,
    reference_case, tolerances(case=...)), so the cases gated above are the ones the GPU is judged on.  Its own numeric bounds
    are the mass conditions the issue states (rows sum to 1 within 1e-4, padded frames exactly zero); this test does not prove
    their absence elsewhere, it pins the plumbing."""
    import test_hip_lstt_stage as G
    assert G.R is R
    src = open(G.__file__).read()
    for stage in R.STAGES:
        assert f"R.tolerances('{stage}', dt" in src and f"R.reference_case('{stage}', dt, case)" in src, stage
    assert src.count('case=case') + src.count('R.DECODE_ROUTES[route], case)') == len(R.STAGES)
    assert [len(R.CASES[s]) for s in R.STAGES] == [10, 2, 1, 2, 3]


@pytest.mark.parametrize('dt', DTS)
def test_stage_weights_round_what_the_pack_rounds(synth_weights, dt):
    """stage_weights against rmem_ocu_amd/pack.py on the CPU: 16-bit tensors of the pack equal the reference's weights exactly,
    fp32 tensors of the pack equal them as fp32 values (biases, norm gains, GroupNorm, depth-wise taps, temporal PE)."""
    from rmem_ocu_amd import _lib
    from rmem_ocu_amd.pack import pack_state_dict
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    e16 = R.E16[dt]
    P, w = pack_state_dict(synth_weights, 'cpu', 3, e16), R.weights(dt)
    nhwc = lambda t: t.permute(0, 2, 3, 1)      # noqa: E731
    pairs = [('proj.w', nhwc(w['encoder_projector.weight'])), ('proj.b', w['encoder_projector.bias']),
             ('pe_cur', w['cur_pos_emb'].reshape(-1)), ('pe_mem', w['mem_pos_emb'].reshape(4, 256))]
    for i in range(3):
        s, d = f'LSTT.layers.{i}', f'l{i}'
        pairs.append((d + '.self_qkv.w', torch.cat([w[f'{s}.self_attn.linear_{n}.weight'] for n in 'QKV'], 0)))
        pairs.append((d + '.self_qkv.b', torch.cat([w[f'{s}.self_attn.linear_{n}.bias'] for n in 'QKV'], 0)))
        for dst, src in (('self_proj', 'self_attn.projection'), ('long_proj', 'long_term_attn.projection'),
                         ('short_proj', 'short_term_attn.projection'), ('linear_Q', 'linear_Q'), ('linear_V', 'linear_V'),
                         ('linear_QMem', 'linear_QMem'), ('linear_VMem', 'linear_VMem'), ('linear1', 'linear1'), ('linear2', 'linear2')):
            pairs += [(f'{d}.{dst}.w', w[f'{s}.{src}.weight']), (f'{d}.{dst}.b', w[f'{s}.{src}.bias'])]
        for dst, src in (('ln1', 'norm1'), ('ln2', 'norm2'), ('ln3', 'norm3'), ('ln4', 'norm4'), ('gn', 'activation.gn')):
            pairs += [(f'{d}.{dst}.g', w[f'{s}.{src}.weight']), (f'{d}.{dst}.b', w[f'{s}.{src}.bias'])]
        pairs.append((d + '.dw.w', w[s + '.activation.conv.weight'].reshape(-1, 25).t()))
        pairs += [(f'dec_norm{i}.g', w[f'LSTT.decoder_norms.{i}.weight']), (f'dec_norm{i}.b', w[f'LSTT.decoder_norms.{i}.bias'])]
    for n in ('conv_in', 'conv_16x', 'conv_8x', 'conv_4x'):
        pairs += [(f'dec.{n}.w', nhwc(w[f'decoder.{n}.conv.weight'])), (f'dec.{n}.b', w[f'decoder.{n}.conv.bias']),
                  (f'dec.{n}.gn.g', w[f'decoder.{n}.gn.weight'])]
    for n in ('adapter_16x', 'adapter_8x', 'adapter_4x', 'conv_out'):
        pairs += [(f'dec.{n}.w', nhwc(w[f'decoder.{n}.weight'])), (f'dec.{n}.b', w[f'decoder.{n}.bias'])]
    n16 = 0
    for name, ref in pairs:
        assert P[name].dtype == (e16 if name.endswith('.w') and P[name].dim() >= 2 and '.dw.' not in name else torch.float32), name
        n16 += P[name].dtype == e16
        assert torch.equal(P[name].double().reshape(ref.shape), ref), name
    assert n16 == 3 * 10 + 8 + 1
    from rmem_ocu_amd.runtime import sine_pos_emb
    assert torch.equal(sine_pos_emb(11, 13).to(e16).double(), R.stage_pos((11, 13), e16).reshape(143, 256))


def test_seeded_state_is_the_chain_tests_state():
    """seeded_lstt_state draws what the chain identity tests always drew: one generator seeded 7; x, then per layer short_K,
    short_V, bank_K, bank_V."""
    B, L, S = 3, 20, 4
    st = R.seeded_lstt_state(B, L, S)
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    assert torch.equal(st['x'], r(B * L, 256))
    for i in range(3):
        assert torch.equal(st['short_K'][i], r(B * L, 256)) and torch.equal(st['short_V'][i], r(B * L, 256))
        assert torch.equal(st['bank_K'][i], r(B * S, L, 256)) and torch.equal(st['bank_V'][i], r(B * S, L, 256))


def test_reference_mass_and_geometry():
    """The reference's block-0 mass: rows sum to 1, frames a shorter bank does not have are exactly zero; the sizes the GPU cases
    use give the token counts they are meant to (143 = 4 * 32 + 15, 153, and 120 for the size that is not aligned)."""
    m = reference_of('lstt', 'bf16')['mass']
    assert m.shape == (3, 143, 5)
    assert (m.sum(-1) - 1).abs().max() < 1e-12
    assert (m[0, :, 1:] == 0).all() and (m[2, :, 2:] == 0).all() and (m[1] > 0).all()
    assert [R.geometry(hw)[2] for hw in ((161, 193), (129, 257), (160, 192))] == [(11, 13), (9, 17), (10, 12)]
    assert R.geometry((161, 193))[:2] == ((41, 49), (21, 25))
    from rmem_ocu_amd.runtime import temporal_slots
    assert [temporal_slots(T) for T in (1, 2, 5, 8)] == [R.O.temporal_slots(T) for T in (1, 2, 5, 8)]
    assert R.O.temporal_slots(5) != list(range(5)) and R.O.temporal_slots(2) == [0, 1]
