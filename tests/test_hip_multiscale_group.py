"""Multi-scale (x flip) testing inside clip groups: the fused cross-scale merge (rmem_logits_post_ms_merge) against an fp32
restatement, against the flip-pair kernel it generalises (bit for bit) and against the composition the per-clip path runs
(rmem_logits_post + rmem_tta_merge); and one GroupEngine per scale + clip_runner.MultiScaleGroupSlot /
evaluator.run_group_multiscale against SequenceEvaluator, the per-clip reference of the protocol (managers/evaluator.py:342-355,
427-441, 484-523).  Sizes: 161 x 193 and 209 x 257 networks (41 x 49 and 53 x 65 logits), 160 x 192 output."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F32 = torch.float32
NC = 11
# (members ((Hi, Wi, flip), ...) in the evaluator's order, Ho, Wo, align_corners, byte offset of the label buffers)
GEOMS = {
    'two scales': (((41, 49, 0), (53, 65, 0)), 160, 192, True, 64),
    'two scales x flip': (((41, 49, 0), (41, 49, 1), (53, 65, 0), (53, 65, 1)), 160, 192, True, 64),
    'one member below 2x': (((41, 49, 0), (53, 65, 0), (100, 120, 1)), 160, 192, True, 64),        # the pixel route for the whole launch
    'ragged, odd offset': (((41, 49, 0), (53, 65, 1)), 161, 190, False, 65),                       # Wo % 4 != 0, buffers at an odd byte
    'one partial tile': (((5, 7, 0), (6, 8, 1)), 13, 27, True, 64),
}
PK = [(1, 2), (3, 10)]                    # (P, keep)
CANARY, TAIL = 0xA5, 4096


def seeded(seed, shape, scale=1.0):
    rng = np.random.Generator(np.random.PCG64([seed, 0x5CA1E5]))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def reference(name, P, keep):
    """(packed logits per member [P, Hi*Wi, 16], merged labels [P, Ho, Wo], near-tie mask [P, Ho, Wo]) on the CPU in fp32: per member
    mask ids above keep, F.interpolate(bilinear), flip back, softmax; the mean in member order; argmax.  Near-tie: the two best
    merged probabilities are closer than 1e-4 * max(1, max |upsampled logit| of any member) -- test_hip_flip_group.py's rule."""
    members, Ho, Wo, ac, _ = GEOMS[name]
    packed, acc, mag = [], None, None
    for a, (Hi, Wi, fl) in enumerate(members):
        lg = seeded(977 + 31 * a + Hi + keep, (P, NC, Hi, Wi)) * 3.0
        pk = torch.zeros(P, Hi * Wi, 16)
        pk[:, :, :NC] = lg.permute(0, 2, 3, 1).reshape(P, -1, NC)
        packed.append(pk)
        ref = lg.clone()
        ref[:, keep + 1:] = -1e10
        up = F.interpolate(ref, size=(Ho, Wo), mode='bilinear', align_corners=ac)
        if fl:
            up = up.flip(-1)
        pr = torch.softmax(up, dim=1)
        acc = pr if acc is None else acc + pr
        m = up[:, :keep + 1].abs().amax(1)
        mag = m if mag is None else torch.maximum(mag, m)
    merged = acc * np.float32(1.0 / len(members))
    top2 = merged.topk(2, dim=1).values
    tie = (top2[:, 0] - top2[:, 1]) < 1e-4 * mag.clamp_min(1.0)
    return packed, merged.argmax(1), tie


def run_kernel(dev, packed, name, P, keep, twin=True):
    """The kernel on P clips; label and twin buffers sit between canary regions at the geometry's byte offset.
    -> (labels [P, Ho, Wo], twin [P, Ho, Wo] or None, (whole label buffer, whole twin buffer))"""
    from rmem_ocu_amd import ops
    members, Ho, Wo, ac, front = GEOMS[name]
    n = P * Ho * Wo
    bufs = [torch.full((front + n + TAIL,), CANARY, dtype=torch.uint8, device=dev) for _ in range(2 if twin else 1)]
    lab = [b[front:front + n].view(P, Ho, Wo) for b in bufs]
    mem = [(pk.to(dev), Hi, Wi, bool(fl)) for pk, (Hi, Wi, fl) in zip(packed, members)]
    ops.run(ops.logits_post_ms_merge(mem, NC, keep, Ho, Wo, ac, lab[0], lab[1] if twin else None, P=P))
    torch.cuda.synchronize()
    return lab[0], (lab[1] if twin else None), bufs


@pytest.mark.parametrize('pk', PK)
@pytest.mark.parametrize('name', list(GEOMS))
def test_ms_merge_vs_fp32(dev, name, pk):
    P, keep = pk
    _, Ho, Wo, _, front = GEOMS[name]
    packed, ref, tie = reference(name, P, keep)
    lab, twin, bufs = run_kernel(dev, packed, name, P, keep)
    got = lab.cpu().long()
    share = tie.float().mean().item()
    print(f'{name} P={P} keep={keep}: near-ties {share:.5f}')
    assert share < 0.01
    assert (got <= keep).all()
    bad = (got != ref) & ~tie
    assert not bad.any(), f'{int(bad.sum())} labels differ away from near-ties ({int(tie.sum())} near-ties among {tie.numel()})'
    assert torch.equal(twin, lab.flip(-1)), 'the twin buffer is not the exact mirror of the label buffer'
    for b in bufs:
        whole = b.cpu()
        assert (whole[:front] == CANARY).all() and (whole[front + P * Ho * Wo:] == CANARY).all(), 'wrote outside its buffer'


@pytest.mark.parametrize('name', list(GEOMS))
def test_ms_merge_without_twin_buffer(dev, name):
    packed = reference(name, 3, 10)[0]
    with_twin = run_kernel(dev, packed, name, 3, 10)[0]
    alone = run_kernel(dev, packed, name, 3, 10, twin=False)[0]
    assert torch.equal(alone, with_twin)


@pytest.mark.parametrize('geom', [(41, 49, 160, 192, True), (41, 49, 161, 190, False), (25, 33, 40, 50, True)])
def test_ms_merge_of_a_flip_pair_is_bit_identical_to_flip_pairs(dev, geom):
    """Two members of one size, flips (0, 1), pointers lg and lg + P rows: rmem_logits_post_flip_pairs bit for bit, on the tile route
    (aligned and ragged) and on the pixel route."""
    from rmem_ocu_amd import ops
    Hi, Wi, Ho, Wo, ac = geom
    P, keep = 3, 6
    lg = torch.zeros(2 * P * Hi * Wi, 16)
    lg[:, :NC] = seeded(55 + Hi, (2 * P * Hi * Wi, NC)) * 3.0
    lg = lg.to(dev)
    pair = torch.full((2 * P, Ho, Wo), CANARY, dtype=torch.uint8, device=dev)
    mine = torch.full((2 * P, Ho, Wo), CANARY, dtype=torch.uint8, device=dev)
    ops.run(ops.logits_post_flip_pairs(lg, nc=NC, keep=keep, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, align_corners=ac, label_u8=pair, rows=2 * P))
    ops.run(ops.logits_post_ms_merge([(lg, Hi, Wi, False), (lg[P * Hi * Wi:], Hi, Wi, True)], NC, keep, Ho, Wo, ac, mine, mine[P:], P=P))
    torch.cuda.synchronize()
    assert torch.equal(mine, pair)


@pytest.mark.parametrize('pk', PK)
@pytest.mark.parametrize('name', ['two scales x flip', 'one member below 2x', 'ragged, odd offset'])
def test_ms_merge_vs_per_clip_composition(dev, name, pk):
    """Against what the per-clip path runs: rmem_logits_post to a full-size fp32 map per member, then rmem_tta_merge.  Same near-tie
    rule (the two differ only by how the compiler contracts the same expressions)."""
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.evaluator import tta_merge
    P, keep = pk
    members, Ho, Wo, ac, _ = GEOMS[name]
    packed, _, tie = reference(name, P, keep)
    lab = run_kernel(dev, packed, name, P, keep)[0]
    full = [torch.empty(P, 1, NC, Ho, Wo, dtype=F32, device=dev) for _ in members]
    for pkd, (Hi, Wi, _), out in zip(packed, members, full):
        d = pkd.to(dev)
        ops.run([ops.logits_post(d[p], ldl=16, nc=NC, keep=keep, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, align_corners=ac, out=out[p]) for p in range(P)])
    comp = torch.stack([tta_merge([f[p] for f in full], [bool(m[2]) for m in members])[0] for p in range(P)])
    torch.cuda.synchronize()
    bad = (lab.cpu() != comp.cpu()) & ~tie
    assert not bad.any(), f'{int(bad.sum())} labels differ from logits_post + tta_merge away from near-ties'


@pytest.mark.parametrize('name', list(GEOMS))
def test_one_clip_alone_equals_clip_0_of_three(dev, name):
    packed = reference(name, 3, 10)[0]
    three, three_twin, _ = run_kernel(dev, packed, name, 3, 10)
    one, one_twin, _ = run_kernel(dev, [pk[:1].contiguous() for pk in packed], name, 1, 10)
    assert torch.equal(one[0], three[0]) and torch.equal(one_twin[0], three_twin[0])


def test_ms_merge_refuses_bad_arguments(dev):
    """The refusals with real device pointers: nothing is launched (canaries stay), and the accepted call then writes."""
    import ctypes as C
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    lg = torch.zeros(2, 9 * 11, 16, device=dev)
    lab = torch.full((2, 33, 43), CANARY, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(ptrs, n_aug=2, P=2, nc=11, keep=6, label=lab.data_ptr()):
        n = len(ptrs)
        return L.rmem_logits_post_ms_merge((C.c_void_p * n)(*ptrs), (C.c_int * n)(*[9] * n), (C.c_int * n)(*[11] * n), (C.c_int * n)(*[0] * n),
                                           n_aug, P, nc, keep, 33, 43, 1, label, None, s)

    ok = [lg.data_ptr(), lg.data_ptr()]
    assert call(ok, n_aug=0) != 0 and call(ok, nc=17) != 0 and call(ok, keep=11) != 0 and call(ok, P=0) != 0
    assert call([lg.data_ptr(), None]) != 0 and call(ok, label=None) != 0 and call([lg.data_ptr(), lg.data_ptr() + 4]) != 0
    torch.cuda.synchronize()
    assert (lab == CANARY).all(), 'a refused call launched'
    assert call(ok) == 0
    torch.cuda.synchronize()
    assert (lab == 0).all()                                                  # equal logits: the first maximum wins


# ---------------------------------------------------------------------------------------------------------- engines + slot
OUT_HW, NETS, N_FRAMES, OBJS = (160, 192), ((161, 193), (209, 257)), 14, 2


def _model(name='r50_aotl'):
    """bank 1 + 2; fitted weights for AOT (skip without them, as test_sequence_evaluator_multiscale_tta), synthetic for DeAOT"""
    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.weights import fitted_state_dict, synth_state_dict
    if name == 'r50_aotl' and not os.path.exists(os.path.join(GOLDEN, 'trained_delta.pt')):
        pytest.skip('fitted weights missing')
    cfg = get_config('pre_vost', 'test', name)
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 2
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(fitted_state_dict(0) if name == 'r50_aotl' else synth_state_dict(0, model='deaot'))
    return model


@functools.lru_cache(maxsize=None)
def _aot_model():
    return _model()


@functools.lru_cache(maxsize=None)
def _clips(count=2, n=N_FRAMES, seed=72):
    """-> (frames[s][c] on the device at both network sizes, first labels [1, 1, Ho, Wo] on the device); the second scale is a
    bilinear resize of the first, the stand-in for the loader's resize that test_sequence_evaluator_multiscale_tta uses"""
    from rmem_ocu_amd.synth import make_clip
    dev = torch.device('cuda', 0)
    frames, firsts = [[], []], []
    for c in range(count):
        f, m = make_clip(seed + c, n, *NETS[0], OBJS)
        frames[0].append(f.to(dev))
        frames[1].append(F.interpolate(f, size=NETS[1], mode='bilinear', align_corners=True).to(dev))
        firsts.append(F.interpolate(m.float(), size=OUT_HW, mode='nearest').to(dev))
    torch.cuda.synchronize()
    return frames, firsts


def _new_object():
    new = torch.zeros(*OUT_HW, dtype=torch.uint8)
    new[OUT_HW[0] // 2:OUT_HW[0] // 2 + OUT_HW[0] // 4, OUT_HW[1] // 8:OUT_HW[1] // 8 + OUT_HW[1] // 5] = OBJS + 1
    return new.cuda(0)


@functools.lru_cache(maxsize=None)
def _evaluator_runs(flip, new_at=None):
    """SequenceEvaluator per clip on both scales -> [(labels [n - 1, Ho, Wo], [(long_memories_indexes, drop trace)] per (scale, flip)
    engine in the evaluator's order)]; new_at: a new object arrives at that frame of clip 0.  Computed once per variant."""
    from rmem_ocu_amd.evaluator import SequenceEvaluator
    frames, firsts = _clips()
    ev = SequenceEvaluator(_aot_model(), 0, flip=flip)
    out = []
    for c in range(len(firsts)):
        labels = {0: firsts[c]}
        if new_at is not None and c == 0:
            labels[new_at] = _new_object().float()[None, None]
        got = ev.run([frames[0][c], frames[1][c]], labels, OUT_HW)
        torch.cuda.synchronize()
        out.append((torch.stack(got).cpu().numpy(), [(list(e.long_memories_indexes), list(e.aot_engines[0].drop_trace)) for e in ev.engines]))
    return out


def _slot_run(model, frames, firsts, flip, lookahead, new_objects=None, feed=None, sync=True):
    """P clips through one GroupEngine per scale + MultiScaleGroupSlot, synchronised after every step (sync), where the twin rows
    of cur_label must be the exact mirror of the plain rows.  -> (labels [P, n, Ho, Wo], engines, bank sizes per step and engine); feed: uint8 [n - 1, P, Ho, Wo]"""
    from rmem_ocu_amd.clip_runner import MultiScaleGroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    dev = torch.device('cuda', 0)
    P = len(firsts)
    engines = [GroupEngine(model, 2 * P if flip else P, 0, lookahead=lookahead, flip_tta=flip) for _ in frames]
    slot = MultiScaleGroupSlot(engines, OUT_HW, dev)
    slot.start(frames, firsts, OBJS, new_objects=new_objects)
    n = int(frames[0][0].shape[0])
    assert tuple(slot.labels.shape[:2]) == (P, n) and tuple(slot.cur_label.shape) == ((2 if flip else 1) * P, *OUT_HW)
    assert all(e.long_term_mem_gap == 5 for e in engines)
    banks = []
    while not slot.done:
        i = slot.cursor
        slot.step(feed=None if feed is None else feed[i - 1])
        if sync:
            slot.synchronize()
            if flip:
                assert torch.equal(slot.cur_label[P:], slot.cur_label[:P].flip(-1)), f'frame {i}: twin rows are not the mirror of the plain rows'
            banks.append([[len(sl) for sl in e.rt.slots] for e in engines])
    slot.synchronize()
    return slot.labels[:, :n].cpu().numpy().copy(), engines, banks


def _check_against_evaluator(got, engines, refs, flip, what):
    P = len(refs)
    for p, (ref_labels, ref_traces) in enumerate(refs):
        agree = (got[p][1:] == ref_labels).mean()
        print(f'{what} clip {p}: label agreement with SequenceEvaluator {agree:.5f}')
        assert agree >= 0.995
        a = 0
        for e in engines:                                  # the evaluator's order: scale outer, flip inner
            for row in ((p, P + p) if flip else (p,)):
                assert (e.long_memories_indexes(row), e.drop_trace[row]) == ref_traces[a], (p, a)
                a += 1
        assert a == len(ref_traces)


@functools.lru_cache(maxsize=None)
def _flip_slot_run():
    frames, firsts = _clips()
    return _slot_run(_aot_model(), frames, firsts, True, 4)


def test_multiscale_flip_group_matches_per_clip_evaluator(dev):
    """Two clips x two scales x flip: two flip groups of four rows and one merge of four members per frame against
    SequenceEvaluator(flip=True).run([f0, f1]) clip by clip: labels, and per engine row the bank index and eviction traces of the
    evaluator's engine for that (scale, flip)."""
    got, engines, _ = _flip_slot_run()
    _check_against_evaluator(got, engines, _evaluator_runs(True), True, 'multi-scale x flip')


def test_multiscale_group_without_flip_lookahead_1(dev):
    frames, firsts = _clips()
    got, engines, _ = _slot_run(_aot_model(), frames, firsts, False, 1)
    _check_against_evaluator(got, engines, _evaluator_runs(False), False, 'multi-scale, look-ahead 1')


def test_multiscale_group_fed_labels(dev):
    """step(feed = the evaluator's own labels): the memories continue from the reference's labels, so every frame is an independent
    comparison; the delivered labels stay the prediction."""
    frames, firsts = _clips()
    refs = _evaluator_runs(True)
    feed = torch.from_numpy(np.stack([r[0] for r in refs], 1)).to(dev)       # [n - 1, P, Ho, Wo]: a frame's labels are contiguous
    torch.cuda.synchronize()
    got, engines, _ = _slot_run(_aot_model(), frames, firsts, True, 4, feed=feed)
    for p, (ref_labels, _) in enumerate(refs):
        per_frame = (got[p][1:] == ref_labels).reshape(len(ref_labels), -1).mean(1)
        print(f'fed labels clip {p}: agreement per frame min {per_frame.min():.5f}')
        assert per_frame.min() >= 0.995
    _check_against_evaluator(got, engines, refs, True, 'fed labels')


def test_multiscale_group_new_object_in_one_clip(dev):
    """A new object's mask arrives at frame 7 of clip 0: in EVERY engine that clip's rows (plain and twin) restart at one bank entry
    from that engine's own frame while clip 1 goes on; labels and traces of SequenceEvaluator.run(labels={0: ..., 7: ...})."""
    frames, firsts = _clips()
    refs = _evaluator_runs(True, 7)
    got, engines, banks = _slot_run(_aot_model(), frames, firsts, True, 4, new_objects={0: (7, _new_object())})
    before, after = banks[5], banks[6]                     # after frames 6 and 7
    for k in range(len(engines)):
        assert before[k][0] == before[k][1] == before[k][2] == before[k][3] > 1, banks
        assert after[k][0] == after[k][2] == 1 and after[k][1] == after[k][3] >= before[k][1], banks
    _check_against_evaluator(got, engines, refs, True, 'new object')
    assert (got[0][7] == OBJS + 1).sum() > 0 and (got[1][7] == OBJS + 1).sum() == 0


def test_run_group_multiscale_never_synchronising_equals_stepwise(dev):
    """evaluator.run_group_multiscale enqueues every step of every engine without a host synchronisation in between; the events
    between the engines' streams alone must order it: the labels of the run that synchronises after every step, byte for byte."""
    from rmem_ocu_amd.evaluator import run_group_multiscale
    frames, firsts = _clips()
    stepwise = _flip_slot_run()[0]
    labels = run_group_multiscale(_aot_model(), frames, firsts, OUT_HW, flip=True, lookahead=4)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (2, N_FRAMES, *OUT_HW)
    assert np.array_equal(labels.cpu().numpy(), stepwise)


def test_multiscale_group_deaot_clip(dev):
    """One 10-frame R50-DeAOTL clip at two scales (group_runtime_deaot, one row per engine) against its SequenceEvaluator run."""
    from rmem_ocu_amd.evaluator import SequenceEvaluator, run_group_multiscale
    model = _model('r50_deaotl')
    frames, firsts = _clips(1, 10, 60)
    ev = SequenceEvaluator(model, 0, flip=False)
    ref = torch.stack(ev.run([frames[0][0], frames[1][0]], {0: firsts[0]}, OUT_HW)).cpu().numpy()
    got = run_group_multiscale(model, frames, firsts, OUT_HW, flip=False, lookahead=4).cpu().numpy()
    agree = (got[0][1:] == ref).mean()
    print(f'deaot multi-scale clip: label agreement with SequenceEvaluator {agree:.5f}')
    assert agree >= 0.995
