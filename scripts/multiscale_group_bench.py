#!/usr/bin/env python
"""Multi-scale + flip test-time augmentation: multi-scale clip groups against the per-clip evaluator.

cfg-2 geometry (480 x 854 video, R50-AOTL, bank 1 + 7, 3 objects), scales [1.0, 1.3], flip on, synthetic weights, clips from
synth.make_clip (the second scale is a bilinear resize of the first).  Reported, in ORIGINAL frames per second (the 2 x 2
augmentations of a frame are one frame):
  (a) multi-scale groups: one GroupEngine(flip_tta=True) per scale with P = --clips clips (2P rows each) under one
      clip_runner.MultiScaleGroupSlot, --slots slots in flight;
  (c) SequenceEvaluator(flip=True).run([frames_s0, frames_s1]), the per-clip path, on the same clips one after the other;
and the device time of rmem_logits_post_ms_merge per step (4 members -> P label rows and their mirrors) against
rmem_logits_post_images on the same rows (2P rows at each of the two sizes, two launches).
Everything is timed with HIP events after a warm-up pass that builds every launch list and graph, --runs times each, alternating.

    python scripts/multiscale_group_bench.py [--clips 4] [--slots 3] [--frames 40] [--runs 3] [--eval-clips 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIDEO_HW, OBJS, SCALES = (480, 854), 3, [1.0, 1.3]


def timed(fn, streams):
    """fn() enqueues (or runs) the work; streams: the streams it runs on besides the current one.  -> milliseconds between two HIP
    events on the current stream, the second recorded behind all of them."""
    cur = torch.cuda.current_stream()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(cur)
    for s in streams:
        s.wait_event(t0)
    fn()
    for s in streams:
        cur.wait_stream(s)
    t1.record(cur)
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=4, help='P: clips per multi-scale slot')
    ap.add_argument('--slots', type=int, default=3, help='multi-scale slots in flight')
    ap.add_argument('--frames', type=int, default=40, help='clip length')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--eval-clips', type=int, default=2, help='clips the per-clip evaluator runs per timed pass')
    ap.add_argument('--kernel-launches', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('multiscale_group_bench.py measures on the GPU: no device found')

    import torch.nn.functional as F
    from rmem_ocu_amd import build_vos_model, get_config, ops
    from rmem_ocu_amd.clip_runner import MultiScaleGroupSlot
    from rmem_ocu_amd.evaluator import SequenceEvaluator
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from rmem_ocu_amd.synth import make_clip, network_size
    from rmem_ocu_amd.weights import synth_state_dict

    dev = torch.device('cuda', 0)
    cfg = get_config('pre_vost', 'bench', 'r50_aotl')
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 7
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0))
    nets = [network_size(*VIDEO_HW, scale=sc) for sc in SCALES]
    P, G, n = args.clips, args.slots, args.frames
    clips, firsts = [], []
    for j in range(2):                                   # two distinct clips, as bench.py
        f, m = make_clip(1000 + j, n, nets[0][0], nets[0][1], OBJS)
        clips.append([f.to(dev)] + [F.interpolate(f, size=hw, mode='bilinear', align_corners=True).to(dev) for hw in nets[1:]])
        firsts.append(F.interpolate(m.float(), size=VIDEO_HW, mode='nearest').to(dev))

    slots = [MultiScaleGroupSlot([GroupEngine(model, 2 * P, 0, 5, lookahead=2, flip_tta=True) for _ in SCALES], VIDEO_HW, dev)
             for _ in range(G)]

    def run_slots():
        for s in slots:
            s.start([[clips[c % 2][k] for c in range(P)] for k in range(len(SCALES))], [firsts[c % 2] for c in range(P)], OBJS)
        while not all(s.done for s in slots):          # interleaved, as bench.py pumps its slots
            for s in slots:
                if not s.done:
                    s.step()

    streams = [st for s in slots for e in s.engines for st in (e.stream, e.enc_stream)]
    ev = SequenceEvaluator(model, 0, flip=True)

    def run_evaluator():
        for c in range(args.eval_clips):
            ev.run(clips[c % 2], {0: firsts[c % 2]}, VIDEO_HW)

    # warm-up: one whole pass of each (every launch list and graph, T = 1..8)
    run_slots(); run_evaluator()
    torch.cuda.synchronize()
    res = {'multiscale_group': [], 'evaluator_multiscale_flip': []}
    for _ in range(args.runs):
        ms = timed(run_slots, streams)
        res['multiscale_group'].append(G * P * (n - 1) / ms * 1e3)
        ms = timed(run_evaluator, [e.aot_engines[0].stream for e in ev.engines if hasattr(e.aot_engines[0], 'stream')])
        res['evaluator_multiscale_flip'].append(args.eval_clips * (n - 1) / ms * 1e3)

    # the post-processing kernels alone, at the slot's shapes
    rts = [e.rt for e in slots[0].engines]
    Ho, Wo = VIDEO_HW
    lgs = [torch.randn(2 * P * rt.H4 * rt.W4, 16, device=dev) * 3.0 for rt in rts]
    lab = torch.empty(2 * P, Ho, Wo, dtype=torch.uint8, device=dev)
    keep, ac = model.max_obj_num, cfg.MODEL_ALIGN_CORNERS
    members = [m for lg, rt in zip(lgs, rts) for m in ((lg, rt.H4, rt.W4, False), (lg[P * rt.H4 * rt.W4:], rt.H4, rt.W4, True))]
    merge_op = ops.logits_post_ms_merge(members, rts[0].nc, keep, Ho, Wo, ac, lab, lab[P:], P=P)
    plain_ops = [ops.logits_post(lg, ldl=16, images=2 * P, nc=rt.nc, keep=keep, Hi=rt.H4, Wi=rt.W4, Ho=Ho, Wo=Wo, align_corners=ac,
                                 label_u8=lab) for lg, rt in zip(lgs, rts)]
    s = torch.cuda.current_stream().cuda_stream
    progs = (('ms_merge_us', [merge_op]), ('logits_post_images_us', plain_ops))
    kern = {name: [] for name, _ in progs}
    for _, prog in progs:
        for _ in range(20):
            ops.run(prog, s)
    for _ in range(args.runs):
        for name, prog in progs:
            ms = timed(lambda: [ops.run(prog, s) for _ in range(args.kernel_launches)], [])
            kern[name].append(ms / args.kernel_launches * 1e3)

    out = {'geometry': {'video': VIDEO_HW, 'networks': [list(hw) for hw in nets], 'logits': [[rt.H4, rt.W4] for rt in rts]},
           'scales': SCALES, 'flip': True, 'clips': P, 'rows_per_engine': 2 * P, 'slots_in_flight': G, 'clip_frames': n,
           'frames_per_s': {k: [round(v, 1) for v in vs] for k, vs in res.items()},
           'kernel': {k: [round(v, 2) for v in vs] for k, vs in kern.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
