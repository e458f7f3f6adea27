#!/usr/bin/env python
"""A clip list of mixed lengths: ragged clip groups against today's equal-length schedule.

cfg-2 geometry (480 x 854 video, R50-AOTL, bank 1 + 7, 3 objects), synthetic weights, frames from synth.make_clip.  The clip list is
--clips clips whose lengths are drawn once with a fixed seed from 34 .. 104 (printed).  The whole job is drained, --engines
engines in flight, in propagated frames per second:
  (a) the equal-length schedule: clip_runner.group_units(lengths, rows), each unit on a GroupSlot of the unit's size (a DAVIS-like
      list gives units of one or two clips);
  (b) ragged groups: --engines RaggedGroupSlots of --rows rows, the clips dealt to them in ClipFeeder(lengths, group=1) order
      (longest first).
Also reported: row occupancy of (b) (row_steps_live over all row-steps), refills, and the device time of rmem_route_labels per
step at the group's shape.  Everything is timed with HIP events after a warm-up pass of each leg that builds every launch list and
graph, --runs times each, alternating.

    python scripts/ragged_group_bench.py [--clips 30] [--rows 8] [--engines 3] [--lookahead 4] [--runs 3] [--leg both|a]

--leg a runs the equal-length schedule alone and uses nothing newer than GroupSlot, so the same file measures it on an older commit.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIDEO_HW, OBJS = (480, 854), 3


def timed(fn, streams):
    """fn() enqueues the work and returns the streams it ran on (or None: ``streams``).  -> milliseconds between two HIP events on
    the current stream, the second recorded behind all of them."""
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
    ap.add_argument('--clips', type=int, default=30)
    ap.add_argument('--rows', type=int, default=8)
    ap.add_argument('--engines', type=int, default=3, help='engines in flight (bench.py: 3 groups of 8)')
    ap.add_argument('--lookahead', type=int, default=4)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--seed', type=int, default=2024)
    ap.add_argument('--kernel-launches', type=int, default=200)
    ap.add_argument('--leg', choices=('both', 'a'), default='both', help='a: the equal-length schedule alone')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ragged_group_bench.py measures on the GPU: no device found')

    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.clip_runner import ClipFeeder, GroupSlot, group_units
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from rmem_ocu_amd.synth import make_clip, network_size
    from rmem_ocu_amd.weights import synth_state_dict

    dev = torch.device('cuda', 0)
    cfg = get_config('pre_vost', 'bench', 'r50_aotl')
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 7
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0))
    net_hw = network_size(*VIDEO_HW)
    lengths = [int(v) for v in np.random.default_rng(args.seed).integers(34, 105, args.clips)]
    print('clip lengths:', lengths, flush=True)
    base = [make_clip(1000 + j, max(lengths), net_hw[0], net_hw[1], OBJS) for j in range(2)]       # two distinct clips, as bench.py
    base = [(f.to(dev), m.to(dev)) for f, m in base]
    clips = [(base[j % 2][0][:n], base[j % 2][1]) for j, n in enumerate(lengths)]                  # clip j: the first n frames
    frames_total = sum(n - 1 for n in lengths)
    G, R, la = args.engines, args.rows, args.lookahead

    # ---- (a) equal-length units, each on a GroupSlot of its size; a lane keeps one slot per unit size
    units = group_units(lengths, R)
    lanes = [{} for _ in range(G)]

    def lane_slot(lane, size):
        if size not in lane:
            lane[size] = GroupSlot(GroupEngine(model, size, 0, 5, lookahead=la), VIDEO_HW, dev)
        return lane[size]

    def run_units():
        todo, cur = list(units), [None] * G
        while True:
            busy = False
            for g in range(G):
                if cur[g] is None or cur[g].done:
                    cur[g] = None
                    if todo:
                        u = todo.pop(0)
                        cur[g] = lane_slot(lanes[g], len(u))
                        cur[g].start([clips[c][0] for c in u], [clips[c][1] for c in u], OBJS)
                if cur[g] is not None and not cur[g].done:
                    cur[g].step()
                    busy = True
            if not busy and not todo:
                return

    def unit_streams():
        return [st for lane in lanes for s in lane.values() for st in (s.engine.stream, s.engine.enc_stream)]

    if args.leg == 'a':
        run_units()
        torch.cuda.synchronize()
        fps = [round(frames_total / timed(run_units, unit_streams()) * 1e3, 1) for _ in range(args.runs)]
        print(json.dumps({'clips': len(lengths), 'lengths': lengths, 'frames_propagated': frames_total, 'engines_in_flight': G,
                          'lookahead': la, 'unit_sizes': sorted({len(u) for u in units}), 'units': len(units),
                          'frames_per_s': {'equal_length_units': fps}}))
        return

    # ---- (b) ragged groups
    from rmem_ocu_amd import _lib, ops
    from rmem_ocu_amd.clip_runner import RaggedGroupSlot
    engines = [GroupEngine(model, R, 0, lookahead=la) for _ in range(G)]
    feeder_order = []
    feeder = ClipFeeder(lengths, group=1)
    while True:
        u = feeder.next_unit()
        if u is None:
            break
        feeder_order += u
    counters = {}
    slots = [RaggedGroupSlot(e, VIDEO_HW, dev) for e in engines]      # kept across passes: the graphs name their label rows

    def run_ragged():
        for s in slots:
            s.row_steps_live = s.row_steps_idle = s.refills = 0
        for k, c in enumerate(feeder_order):
            slots[k % G].submit(c, clips[c][0], clips[c][1])
        finished = 0
        while not all(s.done for s in slots):
            for s in slots:
                if not s.done:
                    finished += len(s.step())
        assert finished == len(lengths)
        live, idle = sum(s.row_steps_live for s in slots), sum(s.row_steps_idle for s in slots)
        assert live == frames_total
        counters.update(row_steps_live=live, row_steps_idle=idle, occupancy=round(live / (live + idle), 4),
                        refills=sum(s.refills for s in slots), group_steps=(live + idle) // R)

    ragged_streams = [st for e in engines for st in (e.stream, e.enc_stream)]

    # warm-up: one whole pass of each leg (every launch list and graph of every engine)
    run_units(); run_ragged()
    torch.cuda.synchronize()
    res = {'equal_length_units': [], 'ragged_groups': []}
    for _ in range(args.runs):
        ms = timed(run_units, unit_streams())
        res['equal_length_units'].append(frames_total / ms * 1e3)
        ms = timed(run_ragged, ragged_streams)
        res['ragged_groups'].append(frames_total / ms * 1e3)

    # ---- the routing kernel alone at the group's shape: every row live, delivering into its own map
    rows_u8 = torch.randint(0, OBJS + 1, (R, *VIDEO_HW), dtype=torch.uint8, device=dev)
    dsts = torch.zeros(R, *VIDEO_HW, dtype=torch.uint8, device=dev)
    lr = ops.LabelRoutes(rows_u8, dev)
    s = torch.cuda.current_stream().cuda_stream
    lr.upload([(dsts[r], None, None, -1, _lib.ROUTE_LIVE) for r in range(R)], s)
    for _ in range(20):
        lr.op(s)
    kern = [timed(lambda: [lr.op(s) for _ in range(args.kernel_launches)], []) / args.kernel_launches * 1e3 for _ in range(args.runs)]

    out = {'geometry': {'video': VIDEO_HW, 'network': list(net_hw)}, 'clips': len(lengths), 'lengths': lengths,
           'frames_propagated': frames_total, 'rows': R, 'engines_in_flight': G, 'lookahead': la,
           'unit_sizes': sorted({len(u) for u in units}), 'units': len(units),
           'frames_per_s': {k: [round(v, 1) for v in vs] for k, vs in res.items()}, 'ragged': counters,
           'route_labels_us_per_step': [round(v, 2) for v in kern]}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
