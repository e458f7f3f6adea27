"""Flip test-time augmentation inside clip groups: the fused pair kernel (rmem_logits_post_flip_pairs) against an fp32
restatement and against the composition the per-clip path runs (rmem_logits_post + rmem_tta_merge), and
GroupEngine(flip_tta=True) + GroupSlot against SequenceEvaluator(flip=True), the per-clip reference of the protocol
(managers/evaluator.py:342-355, 427-441, 484-523)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32 = torch.float32
NC = 11
GEOMS = [(41, 49, 160, 192, True),
         (41, 49, 161, 190, False),      # odd Ho, Wo not a multiple of 4: ragged mirrored stores
         (25, 33, 40, 50, True),         # below 2x: the one-pixel-per-thread route
         (9, 11, 33, 43, True),          # a single partial tile
         (121, 213, 480, 854, True)]     # the bench geometry
PAIRS = [(3, 6), (2, 10), (1, 1)]        # (P, keep)
CANARY, FRONT, TAIL = 0xA5, 64, 4096


def seeded(seed, shape, scale=1.0):
    rng = np.random.Generator(np.random.PCG64([seed, 0xC0FFEE]))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def reference(geom, P, keep):
    """(packed logits [2P, Hi*Wi, 16], merged fp32 labels [P, Ho, Wo], near-tie mask [P, Ho, Wo], share of pixels where the merge
    differs from the plain row alone), on the CPU in fp32: mask ids above keep, F.interpolate(bilinear), softmax,
    0.5 * (plain + twin.flip(-1)), argmax.  Near-tie: the two best merged probabilities are closer than
    1e-4 * max(1, max |upsampled logit| of either member) -- test_logits_label_only_routes_vs_fp32's rounding bound on a blended
    logit, carried through a softmax whose slope is <= 1/4."""
    Hi, Wi, Ho, Wo, ac = geom
    lg = seeded(211 + Hi + keep, (2 * P, NC, Hi, Wi)) * 3.0
    lgn = torch.zeros(2 * P, Hi * Wi, 16)
    lgn[:, :, :NC] = lg.permute(0, 2, 3, 1).reshape(2 * P, -1, NC)
    ref = lg.clone()
    ref[:, keep + 1:] = -1e10
    up = F.interpolate(ref, size=(Ho, Wo), mode='bilinear', align_corners=ac)
    pr = torch.softmax(up, dim=1)
    merged = 0.5 * (pr[:P] + pr[P:].flip(-1))
    top2 = merged.topk(2, dim=1).values
    mag = up[:, :keep + 1].abs().amax(1)
    mag = torch.maximum(mag[:P], mag[P:].flip(-1)).clamp_min(1.0)
    tie = (top2[:, 0] - top2[:, 1]) < 1e-4 * mag
    label = merged.argmax(1)
    changed = (label != pr[:P].argmax(1)).float().mean().item()
    return lgn, label, tie, changed


def run_kernel(dev, lgn, rows, keep, geom):
    """The kernel on `rows` rows of packed logits; the label buffer sits between two canary regions.  -> (labels, whole buffer)"""
    from rmem_ocu_amd import ops
    Hi, Wi, Ho, Wo, ac = geom
    n = rows * Ho * Wo
    buf = torch.full((FRONT + n + TAIL,), CANARY, dtype=torch.uint8, device=dev)
    lab = buf[FRONT:FRONT + n].view(rows, Ho, Wo)
    ops.run(ops.logits_post_flip_pairs(lgn.to(dev), nc=NC, keep=keep, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, align_corners=ac, label_u8=lab, rows=rows))
    torch.cuda.synchronize()
    return lab, buf


@pytest.mark.parametrize('pk', PAIRS)
@pytest.mark.parametrize('geom', GEOMS)
def test_flip_pairs_vs_fp32(dev, geom, pk):
    P, keep = pk
    Ho, Wo = geom[2], geom[3]
    lgn, ref, tie, changed = reference(geom, P, keep)
    lab, buf = run_kernel(dev, lgn, 2 * P, keep, geom)
    got = lab.cpu().long()
    print(f'{geom} P={P} keep={keep}: near-ties {tie.float().mean().item():.5f}, merge changes {changed:.3f} of the plain row\'s labels')
    assert tie.float().mean().item() < 0.01
    assert (got <= keep).all()
    bad = (got[:P] != ref) & ~tie
    assert not bad.any(), f'{int(bad.sum())} labels differ away from near-ties ({int(tie.sum())} near-ties among {tie.numel()})'
    assert torch.equal(got[P:], got[:P].flip(-1)), 'the twin rows are not the exact mirror of the plain rows'
    whole = buf.cpu()
    assert (whole[:FRONT] == CANARY).all() and (whole[FRONT + 2 * P * Ho * Wo:] == CANARY).all(), 'wrote outside label_u8'


@pytest.mark.parametrize('pk', PAIRS)
@pytest.mark.parametrize('geom', GEOMS)
def test_flip_pairs_vs_per_clip_composition(dev, geom, pk):
    """Against what the per-clip path runs today: rmem_logits_post to full-size fp32 logits per row, then rmem_tta_merge of the
    pair.  Same near-tie rule (the two differ only by how the compiler contracts the same expressions)."""
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.evaluator import tta_merge
    P, keep = pk
    Hi, Wi, Ho, Wo, ac = geom
    lgn, _, tie, _ = reference(geom, P, keep)
    lab, _ = run_kernel(dev, lgn, 2 * P, keep, geom)
    lgd = lgn.to(dev)
    full = torch.empty(2 * P, 1, NC, Ho, Wo, dtype=F32, device=dev)
    ops.run([ops.logits_post(lgd[r], ldl=16, nc=NC, keep=keep, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, align_corners=ac, out=full[r]) for r in range(2 * P)])
    comp = torch.stack([tta_merge([full[p], full[P + p]], [False, True])[0] for p in range(P)])
    torch.cuda.synchronize()
    bad = (lab[:P].cpu() != comp.cpu()) & ~tie
    assert not bad.any(), f'{int(bad.sum())} labels differ from logits_post + tta_merge away from near-ties'


@pytest.mark.parametrize('geom', GEOMS)
def test_one_pair_alone_equals_pair_of_three(dev, geom):
    lgn = reference(geom, 3, 6)[0]
    three, _ = run_kernel(dev, lgn, 6, 6, geom)
    one, _ = run_kernel(dev, lgn[[0, 3]].contiguous(), 2, 6, geom)
    assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[3])


def test_flip_pairs_refuses_bad_arguments(dev):
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    lg = torch.zeros(4, 9 * 11, 16, device=dev)
    lab = torch.full((4, 33, 43), CANARY, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(logits, rows, nc, keep, label):
        return L.rmem_logits_post_flip_pairs(logits, rows, nc, keep, 9, 11, 33, 43, 1, label, s)

    assert call(lg.data_ptr(), 3, 11, 6, lab.data_ptr()) != 0 and b'even' in L.rmem_last_error_string()
    assert call(lg.data_ptr(), 4, 17, 6, lab.data_ptr()) != 0
    assert call(lg.data_ptr(), 4, 11, 11, lab.data_ptr()) != 0
    assert call(None, 4, 11, 6, lab.data_ptr()) != 0
    assert call(lg.data_ptr(), 4, 11, 6, None) != 0
    assert call(lg.data_ptr() + 4, 4, 11, 6, lab.data_ptr()) != 0            # the tap rows are read with 16-byte loads
    torch.cuda.synchronize()
    assert (lab == CANARY).all(), 'a refused call launched'
    assert call(lg.data_ptr(), 4, 11, 6, lab.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (lab == 0).all()                                                  # equal logits: the first maximum wins


# ---------------------------------------------------------------------------------------------------------------- engine + slot
def _model(former, latter, name='r50_aotl'):
    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.weights import synth_state_dict
    cfg = get_config('pre_vost', 'test', name)
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = former, latter
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0, model='deaot' if name == 'r50_deaotl' else 'aot'))
    return model


def _first_masks(mask, out_hw, net_hw, dev):
    """The first-frame annotation at the original size (what the evaluator is given) and its nearest resize to the network size by
    the kernel the evaluator itself uses (what the slot is given)."""
    from rmem_ocu_amd import ops
    first = F.interpolate(mask.float(), size=out_hw, mode='nearest').to(dev)
    net = torch.empty(1, 1, *net_hw, dtype=F32, device=dev)
    ops.run(ops.resize_nearest_flip(first.contiguous(), net, flip=False))
    torch.cuda.synchronize()
    return first, net


def _evaluator_runs(model, clips, out_hw, dev, later=None):
    """SequenceEvaluator(flip=True) per clip -> [(labels [n - 1, Ho, Wo], [(long_memories_indexes, drop trace) of its two engines])]"""
    from rmem_ocu_amd.evaluator import SequenceEvaluator
    ev = SequenceEvaluator(model, 0, flip=True)
    out = []
    for c, (frames, first) in enumerate(clips):
        labels = {0: first}
        if later and c in later:
            labels[later[c][0]] = later[c][1]
        got = ev.run(frames, labels, out_hw)
        torch.cuda.synchronize()
        out.append((torch.stack(got).cpu().numpy(), [(list(e.long_memories_indexes), list(e.aot_engines[0].drop_trace)) for e in ev.engines]))
    return out


def _flip_group_run(model, frames, masks, objs, out_hw, dev, lookahead, new_objects=None, feed=None):
    """P clips through GroupEngine(flip_tta=True) + GroupSlot; after every step the twin rows of cur_label must be the exact
    mirror of the plain rows.  -> (labels [P, n, Ho, Wo], engine, bank sizes per step)"""
    from rmem_ocu_amd.clip_runner import GroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    P = len(frames)
    ge = GroupEngine(model, 2 * P, 0, 5, lookahead=lookahead, flip_tta=True)
    gs = GroupSlot(ge, out_hw, dev)
    gs.start(frames, masks, objs, new_objects=new_objects)
    n = int(frames[0].shape[0])
    assert tuple(gs.labels.shape[:2]) == (P, n) and tuple(gs.cur_label.shape) == (2 * P, *out_hw)
    banks = []
    while not gs.done:
        i = gs.cursor
        gs.step(feed=None if feed is None else feed[:, i - 1])
        ge.synchronize()
        assert torch.equal(gs.cur_label[P:], gs.cur_label[:P].flip(-1)), f'frame {i}: twin rows are not the mirror of the plain rows'
        banks.append([len(sl) for sl in ge.rt.slots])
    return gs.labels[:, :n].cpu().numpy().copy(), ge, banks


def _check_against_evaluator(got, ge, refs, what):
    P = len(refs)
    for p, (ref_labels, ref_traces) in enumerate(refs):
        agree = (got[p][1:] == ref_labels).mean()
        print(f'{what} clip {p}: label agreement with SequenceEvaluator(flip=True) {agree:.5f}, indexes {ge.long_memories_indexes(p)} / '
              f'{ge.long_memories_indexes(P + p)}')
        assert agree >= 0.995
        for a, row in enumerate((p, P + p)):
            assert (ge.long_memories_indexes(row), ge.drop_trace[row]) == ref_traces[a], (p, a)


def test_flip_group_matches_per_clip_evaluator(dev):
    """Two clips as two flip pairs on one GroupEngine of four rows against SequenceEvaluator(flip=True) clip by clip: labels, and per
    row the bank index and eviction traces of the evaluator's plain and flipped engines."""
    from rmem_ocu_amd.synth import make_clip
    out_hw, n = (160, 192), 26
    model = _model(1, 2)
    frames, firsts, nets = [], [], []
    for c in range(2):
        f, m = make_clip(40 + c, n, 161, 193, 3)
        first, net = _first_masks(m, out_hw, (161, 193), dev)
        frames.append(f.to(dev)); firsts.append(first); nets.append(net)
    refs = _evaluator_runs(model, list(zip(frames, firsts)), out_hw, dev)
    got, ge, _ = _flip_group_run(model, frames, nets, 3, out_hw, dev, lookahead=4)
    _check_against_evaluator(got, ge, refs, 'flip group')


def test_flip_group_from_pinned_uint8_frames(dev):
    """Flip pairs fed from pinned uint8 frames (one H2D copy and one ingest per frame, the twin mirrored from the ingested frame on
    the device) give exactly the labels of the same pairs fed with the ingested fp32 frames from device memory -- the bar of
    test_group_slot_from_pinned_uint8_frames -- with and without encoder look-ahead."""
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.synth import make_clip
    n = 9
    model = _model(1, 2)
    u8s, ings, masks = [], [], []
    for c in range(2):
        f, m = make_clip(40 + c, n, 161, 193, 2)
        vid = F.interpolate(f, size=(160, 192), mode='bilinear', align_corners=False)
        u8 = (vid * 40.0 + 128.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()
        u8d = u8.to(dev)
        ing = torch.empty(n, 3, 161, 193, dtype=F32, device=dev)
        ops.run([ops.ingest_rgb8(u8d[i], Hs=160, Ws=192, Hd=161, Wd=193, out_chw=ing[i]) for i in range(n)])
        u8s.append(u8); ings.append(ing); masks.append(m.to(dev))
    torch.cuda.synchronize()
    for la in (2, 1):
        a = _flip_group_run(model, ings, masks, 2, (160, 192), dev, lookahead=la)[0]
        b = _flip_group_run(model, u8s, masks, 2, (160, 192), dev, lookahead=la)[0]
        assert np.array_equal(a[:, 1:], b[:, 1:]), f'look-ahead {la}'


def test_flip_group_from_jpeg_clips(dev):
    """Flip pairs fed from JpegClips (decoded once on the device, the twin mirrored from the ingested frame) give exactly the labels
    of the same frames decoded on the host into pinned uint8."""
    from rmem_ocu_amd.jpeg import JpegClip
    from test_hip_jpeg import _jpeg_clip_frames
    n = 9
    model = _model(1, 2)
    clips = [_jpeg_clip_frames(60 + c, n) for c in range(2)]
    masks = [m.to(dev) for _, _, m in clips]
    a = _flip_group_run(model, [d for _, d, _ in clips], masks, 2, (160, 192), dev, lookahead=2)[0]
    jc = [JpegClip(j) for j, _, _ in clips]
    b = _flip_group_run(model, jc, masks, 2, (160, 192), dev, lookahead=2)[0]
    for s in jc:
        s.check(dev)
    assert np.array_equal(a[:, 1:], b[:, 1:])


def test_flip_group_new_object_in_one_pair(dev):
    """A new object's mask arrives at frame 15 of clip 0 of two flip pairs: the overlay goes onto the plain row, its mirror onto the
    twin's, both rows are re-initialised from that frame (the twin from the mirrored frame), so the banks of rows 0 and 2 restart
    at one entry while rows 1 and 3 go on; labels and traces of SequenceEvaluator(flip=True).run(labels={0: ..., 15: ...})."""
    from rmem_ocu_amd.synth import make_clip
    (oh, ow), n, objs = (160, 192), 30, 2
    model = _model(1, 7)
    new = torch.zeros(oh, ow, dtype=torch.uint8)
    new[oh // 2:oh // 2 + oh // 4, ow // 8:ow // 8 + ow // 5] = objs + 1
    frames, firsts, nets = [], [], []
    for c in range(2):
        f, m = make_clip(80 + c, n, 161, 193, objs)
        first, net = _first_masks(m, (oh, ow), (161, 193), dev)
        frames.append(f.to(dev)); firsts.append(first); nets.append(net)
    refs = _evaluator_runs(model, list(zip(frames, firsts)), (oh, ow), dev, later={0: (15, new.to(dev).float()[None, None])})
    got, ge, banks = _flip_group_run(model, frames, nets, objs, (oh, ow), dev, lookahead=2, new_objects={0: (15, new.to(dev))})
    before, after = banks[13], banks[14]                   # after frames 14 and 15
    assert before[0] == before[1] == before[2] == before[3] > 1, banks
    assert after[0] == after[2] == 1 and after[1] == after[3] >= before[1], banks
    _check_against_evaluator(got, ge, refs, 'new object')
    assert (got[0][15] == objs + 1).sum() > 0 and (got[1][15] == objs + 1).sum() == 0


def test_flip_group_deaot_pair(dev):
    """One 12-frame flip pair on an R50-DeAOTL model (group_runtime_deaot) against SequenceEvaluator(flip=True) on the same model."""
    from rmem_ocu_amd.synth import make_clip
    out_hw, n = (160, 192), 12
    model = _model(1, 2, 'r50_deaotl')
    f, m = make_clip(60, n, 161, 193, 3)
    first, net = _first_masks(m, out_hw, (161, 193), dev)
    refs = _evaluator_runs(model, [(f.to(dev), first)], out_hw, dev)
    got, ge, _ = _flip_group_run(model, [f.to(dev)], [net], 3, out_hw, dev, lookahead=4)
    _check_against_evaluator(got, ge, refs, 'deaot flip group')
