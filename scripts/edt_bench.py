"""Distance-transform measurements (rmem_ocu_amd.distance: label_edt, hausdorff2; evaluator.next_clicks); bench.py is not involved.

Stacks of 64 x 480 x 854, 16 x 1080 x 1920 and 1 x 1080 x 1920 uint8 labels (the last shows whether the column pass, one thread
per column, starves on a single frame) in six contents:
  * blobs    seeded blob annotations with 10 objects (tests/census_ref.blobs), every other value, border;
  * disk     one disk of radius H / 2 - 1 on background: the deepest scans of that mode;
  * noise    every pixel uniform over 4 values: every answer is next door;
  * present  distance to value 1 of the blobs;
  * corner   distance to a value that one pixel in the last corner holds: the longest scans of that mode;
  * absent   distance to a value no pixel holds: the sentinel fill.
Per case the median ms of `--iters` calls of label_edt timed one by one with HIP events after `--warmup` calls, on one stream, next
to two yardsticks from the same run:
  (a) a device pass that moves the bytes the transform must move at least, 1 B read and 4 B written per pixel (a uint8 -> int32
      copy of the stack): the memory floor;
  (b) scipy.ndimage.distance_transform_edt on the first frame on the host (tests/edt_ref.edt: per value for the first mode),
      scaled by n; one thread.
hausdorff2 and next_clicks at 10 objects are timed end to end on a host clock, readback included, on the 64-frame stack.
Not measured: the split between the two passes, the spread between runs.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import census_ref  # noqa: E402
import edt_ref as R  # noqa: E402

STACKS = ((64, 480, 854), (16, 1080, 1920), (1, 1080, 1920))
CONTENTS = ('blobs', 'disk', 'noise', 'present', 'corner', 'absent')
MODE = {'blobs': (None, True), 'disk': (None, True), 'noise': (None, True), 'present': (1, False), 'corner': (200, False),
        'absent': (201, False)}


def make_stack(content, n, H, W):
    if content == 'noise':
        return np.random.default_rng(H + W).integers(0, 4, (n, H, W)).astype(np.uint8)
    if content == 'disk':
        y, x = np.mgrid[0:H, 0:W]
        disk = ((y - H // 2) ** 2 + (x - W // 2) ** 2 <= (H // 2 - 1) ** 2).astype(np.uint8)
        return np.broadcast_to(disk, (n, H, W)).copy()
    a = census_ref.blobs(1000 + H, n, H, W)
    if content == 'corner':
        a[:, H - 1, W - 1] = 200
    return a


def device_ms(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def host_ms(torch, fn, warmup, iters):
    times = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edt_bench.json'))
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import distance
    from rmem_ocu_amd.evaluator import next_clicks
    dev = torch.device('cuda', 0)
    res = {'metric': 'label_edt', 'warmup': args.warmup, 'iters': args.iters, 'host_threads': 1, 'cases': []}
    scipy_ms = {}
    for n, H, W in STACKS:
        for content in CONTENTS:
            value, border = MODE[content]
            host = make_stack(content, n, H, W)
            stack = torch.from_numpy(host).to(dev)
            out = torch.empty(stack.shape, dtype=torch.int32, device=dev)
            if (H, W, content) not in scipy_ms:                     # the first frames of the 1080p stacks are the same frame
                t0 = time.perf_counter()
                want = R.edt(host[0], value, border)
                scipy_ms[(H, W, content)] = (time.perf_counter() - t0) * 1e3
                got = distance.label_edt(stack[0], value, border).cpu().numpy()
                assert np.array_equal(got, want), (content, H, W)
            edt = device_ms(torch, lambda: distance.label_edt(stack, value, border, out=out), args.warmup, args.iters)
            floor = device_ms(torch, lambda: out.copy_(stack), args.warmup, args.iters)
            frame_ms = scipy_ms[(H, W, content)]
            res['cases'].append(dict(stack=f'{n}x{H}x{W}', content=content, value=value, border=border, edt_ms=round(edt, 4),
                                     floor_ms=round(floor, 4), scipy_frame_ms=round(frame_ms, 2), edt_over_floor=round(edt / floor, 1),
                                     scipy_over_edt=round(frame_ms * n / edt, 1), equals_scipy_on_frame_0=True))
            print(json.dumps(res['cases'][-1]), file=sys.stderr, flush=True)
            del stack, out
    n, H, W = STACKS[0]
    gt = census_ref.blobs(1000 + H, n, H, W)
    pred = np.zeros_like(gt)
    pred[:, 3:, 5:] = gt[:, :-3, :-5]
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    res['hausdorff_10_objects_ms'] = round(host_ms(torch, lambda: distance.hausdorff(d_pred, d_gt, 10), 1, 5), 2)
    res['next_clicks_10_objects_ms'] = round(host_ms(torch, lambda: next_clicks(d_pred, d_gt, 10), 1, 5), 2)
    res['end_to_end_stack'] = f'{n}x{H}x{W}'
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
