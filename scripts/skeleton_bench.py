"""Thinning measurements (rmem_ocu_amd.skeleton: thin; evaluator.next_scribbles); bench.py is not involved.

Stacks of 64 x 480 x 854, 16 x 1080 x 1920 and 1 x 1080 x 1920 uint8 labels in four contents:
  * blobs    seeded blob annotations with 10 objects (tests/census_ref.blobs);
  * disk     one disk of radius H / 2 - 1 on background: the deepest case, about H / 2 iterations;
  * noise    every pixel uniform over 4 values: a few iterations;
  * thin     an already-thin stack, the skeleton of the blobs: one batch that changes nothing.
Per case the median ms of `--iters` calls of skeleton.thin (to the fixed point, batches of 64 sub-iterations, the 8-byte-per-frame
readback of every batch included) timed one by one with HIP events after `--warmup` calls, on one stream, with the idle-tile skip
and, through RMEM_THIN_SKIP=0 in the same process, without it; the iterations (counted once by calls of two sub-iterations), the
batches, rounds and launches that follow from them; and two yardsticks from the same run:
  (a) a uint8 -> uint8 device copy of the stack: the memory floor of one round;
  (b) the numpy restatement (tests/skeleton_ref) on the first frame: the mean of its first four sub-iterations (after one
      untimed), times the sub-iterations the case needs, times n -- an estimate; at 480 x 854 the whole run on frame 0 is timed as
      well, scaled by n, and compared with the device's frame 0.
evaluator.next_scribbles at 10 objects is timed end to end on a host clock, readback and host paths included, on the 64-frame
blobs moved by (3, 5).  Not measured: the spread between runs, the split between load, sub-iterations and store inside a round,
other tile sizes or sub-iterations per launch.  Prints one JSON line and writes it to --out.
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
import skeleton_ref as R  # noqa: E402

STACKS = ((64, 480, 854), (16, 1080, 1920), (1, 1080, 1920))
CONTENTS = ('blobs', 'disk', 'noise', 'thin')
BATCH = 64


def make_stack(content, n, H, W):
    if content == 'noise':
        return np.random.default_rng(H + W).integers(0, 4, (n, H, W)).astype(np.uint8)
    if content == 'disk':
        y, x = np.mgrid[0:H, 0:W]
        disk = ((y - H // 2) ** 2 + (x - W // 2) ** 2 <= (H // 2 - 1) ** 2).astype(np.uint8)
        return np.broadcast_to(disk, (n, H, W)).copy()
    return census_ref.blobs(1000 + H, n, H, W)


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


def iterations_of(skeleton, stack):
    """the iterations the slowest frame needs, the one that deletes nothing included: calls of one iteration until none loses"""
    work = stack.clone()
    it = 0
    while True:
        it += 1
        before = int((work != 0).sum())
        skeleton.thin(work, max_iterations=1, out=work)
        if int((work != 0).sum()) == before:
            return it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skeleton_bench.json'))
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import skeleton
    from rmem_ocu_amd.evaluator import next_scribbles
    dev = torch.device('cuda', 0)
    th, tw, k = skeleton.tile()
    res = {'metric': 'skeleton_thin', 'warmup': args.warmup, 'iters': args.iters, 'host_threads': 1, 'tile': [th, tw, k], 'batch': BATCH,
           'cases': []}
    numpy_sub_ms, numpy_full_ms = {}, {}
    for n, H, W in STACKS:
        for content in CONTENTS:
            if content == 'thin':
                stack = thin_dev
                host0 = thin_dev[0].cpu().numpy()
            else:
                host = make_stack(content, n, H, W)
                stack = torch.from_numpy(host).to(dev)
                host0 = host[0]
            out = torch.empty_like(stack)
            its = iterations_of(skeleton, stack)
            if (H, W, content) not in numpy_sub_ms:                   # the first frames of the 1080p stacks are the same frame
                R.run(host0, 0, 1)                                  # numpy's first touch of its temporaries is not the yardstick
                t0 = time.perf_counter()
                R.run(host0, 0, 4)
                numpy_sub_ms[(H, W, content)] = (time.perf_counter() - t0) * 1e3 / 4
                if H == 480:
                    t0 = time.perf_counter()
                    want = R.thin(host0)
                    numpy_full_ms[(H, W, content)] = (time.perf_counter() - t0) * 1e3
                    assert np.array_equal(skeleton.thin(stack[0]).cpu().numpy(), want), (content, H, W)
            os.environ.pop('RMEM_THIN_SKIP', None)
            ms = device_ms(torch, lambda: skeleton.thin(stack, batch=BATCH, out=out), args.warmup, args.iters)
            first = out.clone()
            os.environ['RMEM_THIN_SKIP'] = '0'
            ms_off = device_ms(torch, lambda: skeleton.thin(stack, batch=BATCH, out=out), args.warmup, args.iters)
            os.environ.pop('RMEM_THIN_SKIP', None)
            assert torch.equal(first, out), (content, n, H, W)
            if content == 'blobs':
                thin_dev = first
            floor = device_ms(torch, lambda: out.copy_(stack), args.warmup, args.iters)
            batches = -(-2 * its // BATCH)
            rounds = batches * (BATCH // k)
            sub_ms = numpy_sub_ms[(H, W, content)]
            case = dict(stack=f'{n}x{H}x{W}', content=content, thin_ms=round(ms, 4), thin_noskip_ms=round(ms_off, 4),
                        floor_ms=round(floor, 4), iterations=its, batches=batches, rounds=rounds, launches=rounds + batches,
                        ms_per_needed_subiteration=round(ms / (2 * its), 5), round_over_floor=round(ms / rounds / floor, 2),
                        subiteration_over_floor=round(ms / (batches * BATCH) / floor, 3), skip_speedup=round(ms_off / ms, 2),
                        numpy_subiteration_frame_ms=round(sub_ms, 2), numpy_estimate_over_thin=round(sub_ms * 2 * its * n / ms, 1))
            if (H, W, content) in numpy_full_ms:
                full = numpy_full_ms[(H, W, content)]
                case.update(numpy_frame_ms=round(full, 1), numpy_over_thin=round(full * n / ms, 1), equals_numpy_on_frame_0=True)
            res['cases'].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del stack, out, first
        del thin_dev
    n, H, W = STACKS[0]
    gt = census_ref.blobs(1000 + H, n, H, W)
    pred = np.zeros_like(gt)
    pred[:, 3:, 5:] = gt[:, :-3, :-5]
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    res['next_scribbles_10_objects_ms'] = round(host_ms(torch, lambda: next_scribbles(d_pred, d_gt, 10), 1, 3), 2)
    res['next_scribbles_count'] = sum(len(f) for f in next_scribbles(d_pred, d_gt, 10))
    res['end_to_end_stack'] = f'{n}x{H}x{W}'
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
