#!/usr/bin/env python
"""Flip test-time augmentation: clip groups of flip pairs against plain clip groups and against the per-clip evaluator.

cfg-2 geometry (480 x 854 video, R50-AOTL, bank 1 + 7, 3 objects), synthetic weights, clips from synth.make_clip.  Reported, in
ORIGINAL frames per second (a flip pair's two rows are one frame):
  (a) flip groups: GroupEngine(flip_tta=True) with P = --pairs pairs (2P rows), --groups groups in flight;
  (b) plain groups of 2P clips on the same build, the same number of groups in flight;
  (c) SequenceEvaluator(flip=True), the per-clip path, on the same clips one after the other;
and the device time of rmem_logits_post_flip_pairs per group step against rmem_logits_post_images on the same 2P rows.
Everything is timed with HIP events after a warm-up pass that builds every launch list and graph, --runs times each, alternating.

    python scripts/flip_group_bench.py [--pairs 4] [--groups 3] [--frames 40] [--runs 3] [--eval-clips 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIDEO_HW, OBJS = (480, 854), 3


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
    ap.add_argument('--pairs', type=int, default=4)
    ap.add_argument('--groups', type=int, default=3, help='groups in flight (bench.py: 24 clips in flight = 3 groups of 8)')
    ap.add_argument('--frames', type=int, default=40, help='clip length')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--eval-clips', type=int, default=2, help='clips the per-clip evaluator runs per timed pass')
    ap.add_argument('--kernel-launches', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('flip_group_bench.py measures on the GPU: no device found')

    from rmem_ocu_amd import build_vos_model, get_config, ops
    from rmem_ocu_amd.clip_runner import GroupSlot
    from rmem_ocu_amd.evaluator import SequenceEvaluator
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from rmem_ocu_amd.synth import make_clip, network_size
    from rmem_ocu_amd.weights import synth_state_dict

    dev = torch.device('cuda', 0)
    cfg = get_config('pre_vost', 'bench', 'r50_aotl')
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 7
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0))
    net_hw = network_size(*VIDEO_HW)
    P, G, n = args.pairs, args.groups, args.frames
    clips = [make_clip(1000 + j, n, net_hw[0], net_hw[1], OBJS) for j in range(2)]       # two distinct clips, as bench.py
    clips = [(f.to(dev), m.to(dev)) for f, m in clips]
    firsts = [torch.nn.functional.interpolate(m.float(), size=VIDEO_HW, mode='nearest') for _, m in clips]

    def group_slots(flip):
        slots = []
        for _ in range(G):
            eng = GroupEngine(model, 2 * P, 0, 5, lookahead=2, flip_tta=flip)
            slots.append(GroupSlot(eng, VIDEO_HW, dev))
        return slots

    def run_groups(slots):
        k = slots[0].clips
        for s in slots:
            s.start([clips[c % 2][0] for c in range(k)], [clips[c % 2][1] for c in range(k)], OBJS)
        while not all(s.done for s in slots):          # interleaved, as bench.py pumps its slots
            for s in slots:
                if not s.done:
                    s.step()

    def streams_of(slots):
        return [st for s in slots for st in (s.engine.stream, s.engine.enc_stream)]

    flip_slots, plain_slots = group_slots(True), group_slots(False)
    ev = SequenceEvaluator(model, 0, flip=True)

    def run_evaluator():
        for c in range(args.eval_clips):
            ev.run(clips[c % 2][0], {0: firsts[c % 2]}, VIDEO_HW)

    # warm-up: one whole pass of each (every launch list and graph, T = 1..8)
    run_groups(flip_slots); run_groups(plain_slots); run_evaluator()
    torch.cuda.synchronize()
    res = {'flip_group': [], 'plain_group': [], 'evaluator_flip': []}
    for _ in range(args.runs):
        ms = timed(lambda: run_groups(flip_slots), streams_of(flip_slots))
        res['flip_group'].append(G * P * (n - 1) / ms * 1e3)
        ms = timed(lambda: run_groups(plain_slots), streams_of(plain_slots))
        res['plain_group'].append(G * 2 * P * (n - 1) / ms * 1e3)
        ms = timed(run_evaluator, [e.aot_engines[0].stream for e in ev.engines if hasattr(e.aot_engines[0], 'stream')])
        res['evaluator_flip'].append(args.eval_clips * (n - 1) / ms * 1e3)

    # the post-processing kernels alone, at the group's shapes
    rt = flip_slots[0].engine.rt
    rows, Ho, Wo = 2 * P, VIDEO_HW[0], VIDEO_HW[1]
    lg = torch.randn(rows, rt.H4 * rt.W4, 16, device=dev) * 3.0
    lab = torch.empty(rows, Ho, Wo, dtype=torch.uint8, device=dev)
    kw = dict(nc=rt.nc, keep=model.max_obj_num, Hi=rt.H4, Wi=rt.W4, Ho=Ho, Wo=Wo, align_corners=cfg.MODEL_ALIGN_CORNERS, label_u8=lab)
    pair_op = ops.logits_post_flip_pairs(lg, rows=rows, **kw)
    plain_op = ops.logits_post(lg, ldl=16, images=rows, **kw)
    s = torch.cuda.current_stream().cuda_stream
    kern = {'flip_pairs_us': [], 'logits_post_images_us': []}
    for op in (pair_op, plain_op):
        for _ in range(20):
            op(s)
    for _ in range(args.runs):
        for name, op in (('flip_pairs_us', pair_op), ('logits_post_images_us', plain_op)):
            ms = timed(lambda: [op(s) for _ in range(args.kernel_launches)], [])
            kern[name].append(ms / args.kernel_launches * 1e3)

    out = {'geometry': {'video': VIDEO_HW, 'network': list(net_hw), 'logits': [rt.H4, rt.W4]}, 'pairs': P, 'rows': rows,
           'groups_in_flight': G, 'clip_frames': n, 'frames_per_s': {k: [round(v, 1) for v in vs] for k, vs in res.items()},
           'kernel': {k: [round(v, 2) for v in vs] for k, vs in kern.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
