"""Clip scoring measurements (rmem_clip_score_counts through evaluator.clip_counts); bench.py is not involved.

64 seeded frames of blob label maps, the prediction = the annotation shifted by half the dilation radius and speckled, at 480x854
with 10 objects and at 1080x1920 with 5 objects:
  * device frames/s and us per frame: HIP events around `--iters` clip_counts calls on the 64-frame stack after `--warmup` calls
    (labels already on the device, counts left on the device);
  * the same frames through the numpy / scipy restatement the tests compare against (tests/boundary_ref.py), on one process and
    on `--threads` processes (default 16); it is slow, so `--cpu-frames-1` / `--cpu-frames-n` frames of the stack are timed;
  * bytes per frame: the floor of reading both label maps once, the bit planes written, and the bound on plane bytes read back
    (every plane once plus the halo rows; ids without a boundary and tiles without a boundary word are not read).
The device counts of the CPU-timed frames are compared with the restatement's.  Prints one JSON line.  Kernel split: run it under
`rocprofv3 --kernel-trace --stats -- python scripts/boundary_bench.py --skip-cpu`.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import boundary_ref as R  # noqa: E402

FRAMES = 64
CASES = (dict(H=480, W=854, objects=10), dict(H=1080, W=1920, objects=5))


def make_stack(H, W, objects, n):
    r = R.radius(H, W)
    gts = np.stack([R.blobs(H, W, objects + 1, seed=1000 + H + i) for i in range(n)])
    preds = np.stack([R.shifted_speckled(gts[i], r // 2, -(r // 2) + (i % 3), seed=i, speckles=H * W // 4000) for i in range(n)])
    return preds, gts


def _cpu_frame(args):
    return R.frame_counts(*args)


def cpu_rate(preds, gts, num_ids, frames, workers):
    work = [(preds[i], gts[i], num_ids) for i in range(frames)]
    t0 = time.perf_counter()
    if workers == 1:
        out = [_cpu_frame(w) for w in work]
    else:
        with ProcessPoolExecutor(workers) as ex:
            out = list(ex.map(_cpu_frame, work))
    return frames / (time.perf_counter() - t0), np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cpu-frames-1', type=int, default=1)
    ap.add_argument('--cpu-frames-n', type=int, default=16)
    ap.add_argument('--skip-cpu', action='store_true')
    args = ap.parse_args()
    res = {'metric': 'clip_score_counts', 'frames': FRAMES, 'cpu_workers': args.threads, 'cases': []}
    stacks, cpu = [], []
    for c in CASES:                                           # the host work first: its worker processes never see the device
        preds, gts = make_stack(c['H'], c['W'], c['objects'], FRAMES)
        stacks.append((preds, gts))
        if args.skip_cpu:
            cpu.append(None)
            continue
        r1, _ = cpu_rate(preds, gts, c['objects'] + 1, args.cpu_frames_1, 1)
        rn, ref = cpu_rate(preds, gts, c['objects'] + 1, args.cpu_frames_n, args.threads)
        cpu.append((r1, rn, ref))
        print(json.dumps(dict(size=f"{c['H']}x{c['W']}", cpu_1=r1, cpu_n=rn)), file=sys.stderr, flush=True)
    import torch
    from rmem_ocu_amd import evaluator
    dev = torch.device('cuda', 0)
    for c, (preds, gts), cp in zip(CASES, stacks, cpu):
        H, W, num_ids = c['H'], c['W'], c['objects'] + 1
        p, g = torch.from_numpy(preds).to(dev), torch.from_numpy(gts).to(dev)
        for _ in range(args.warmup):
            counts = evaluator.clip_counts(p, g, num_ids)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            counts = evaluator.clip_counts(p, g, num_ids)
        b.record()
        torch.cuda.synchronize()
        sec = a.elapsed_time(b) / 1e3 / args.iters
        plane = 2 * num_ids * H * ((W + 63) // 64) * 8
        halo = (16 + 2 * R.radius(H, W)) / 16 * 18 / 16
        r = dict(size=f'{H}x{W}', objects=c['objects'], radius=R.radius(H, W), device_frames_per_s=round(FRAMES / sec, 1),
                 device_us_per_frame=round(1e6 * sec / FRAMES, 2), ms_per_call=round(1e3 * sec, 3),
                 label_bytes_per_frame_floor=2 * H * W, plane_bytes_written_per_frame=plane,
                 plane_bytes_read_per_frame_bound=int(plane * (1 + halo)),
                 floor_us_per_frame_at_6p3_TBps=round(2 * H * W / 6.3e6, 3))
        if cp is not None:
            r1, rn, ref = cp
            got = counts.cpu().numpy()[:ref.shape[0]]
            r.update(cpu_frames_per_s_1=round(r1, 4), cpu_frames_per_s_n=round(rn, 3), cpu_frames_timed=[args.cpu_frames_1, args.cpu_frames_n],
                     speedup_vs_cpu_1=round(FRAMES / sec / r1, 0), speedup_vs_cpu_n=round(FRAMES / sec / rn, 0),
                     counts_equal_restatement=bool(np.array_equal(got, ref)))
        res['cases'].append(r)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
