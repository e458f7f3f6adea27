"""Nearest-site transform measurements (rmem_ocu_amd.distance: nearest, grow; evaluator.fill_void, labels_from_seeds); bench.py is
not involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels, five cases:
  * nearest         seeded blob annotations with 10 objects (tests/census_ref.blobs), sites = the objects, index and dist2;
  * grow_r4         the same stack, the objects grown over the background by 4 pixels (max_d2 16): scans of at most 4 columns;
  * grow            the same without a limit;
  * fill_void       a one-pixel rim of 255 round every blob, every 255 replaced by the nearest other value: two of three rows
                    hold no pixel to fill;
  * seeds           20 one-pixel seeds per frame grown into a full label map (labels_from_seeds): the long-scan case.
Per case the median ms of `--iters` calls timed one by one with HIP events after `--warmup` calls, on one stream, next to three
yardsticks from the same run:
  (a) a uint8 -> int32 copy of the stack, 1 B read and 4 B written per pixel: the memory floor of a call that writes one map;
  (b) distance.label_edt(value=1) on the stack's site mask (1 where the case has a site, else 0): the same sites, the distance
      alone -- what carrying the index costs;
  (c) scipy.ndimage.distance_transform_edt(return_indices=True) on the first frame on the host, scaled by n; one thread.
Frame 0 of every case is compared with the host: dist2 equals scipy's, the site scipy returns is as near as ours and never comes
before it in raster order, and the grown frame equals a gather at our index.
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

STACKS = ((64, 480, 854), (16, 1080, 1920))
CASES = ('nearest', 'grow_r4', 'grow', 'fill_void', 'seeds')
OBJECTS = tuple(range(1, 11))


def make_stack(case, n, H, W):
    """(the stack, the values that are sites)"""
    if case == 'seeds':
        rng = np.random.default_rng(H + W)
        a = np.zeros((n, H, W), dtype=np.uint8)
        for f in range(n):
            p = rng.choice(H * W, 20, replace=False)
            a[f].reshape(-1)[p] = np.arange(1, 21, dtype=np.uint8)
        return a, tuple(range(1, 256))
    a = census_ref.blobs(1000 + H, n, H, W)
    if case != 'fill_void':
        return a, OBJECTS
    for v in OBJECTS:
        m = a == v
        inner = m.copy()
        inner[:, 1:, :] &= m[:, :-1, :]
        inner[:, :-1, :] &= m[:, 1:, :]
        inner[:, :, 1:] &= m[:, :, :-1]
        inner[:, :, :-1] &= m[:, :, 1:]
        a[m & ~inner] = 255
    return a, tuple(range(255))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nearest_bench.json'))
    args = ap.parse_args()
    import torch
    from scipy.ndimage import distance_transform_edt
    from rmem_ocu_amd import distance
    from rmem_ocu_amd.evaluator import fill_void, labels_from_seeds
    dev = torch.device('cuda', 0)
    res = {'metric': 'label_nearest', 'warmup': args.warmup, 'iters': args.iters, 'host_threads': 1, 'cases': []}
    scipy_ms = {}
    for n, H, W in STACKS:
        for case in CASES:
            host, sites = make_stack(case, n, H, W)
            stack = torch.from_numpy(host).to(dev)
            mask = torch.from_numpy(np.isin(host, sites).astype(np.uint8)).to(dev)
            out32 = torch.empty(stack.shape, dtype=torch.int32, device=dev)
            out8 = torch.empty_like(stack)
            fn = {'nearest': lambda: distance.nearest(stack, sites),
                  'grow_r4': lambda: distance.grow(stack, (0,), sites, max_distance=4, out=out8),
                  'grow': lambda: distance.grow(stack, (0,), sites, out=out8),
                  'fill_void': lambda: fill_void(stack),
                  'seeds': lambda: labels_from_seeds(stack)}[case]
            site0 = np.isin(host[0], sites)
            t0 = time.perf_counter()
            d, (iy, ix) = distance_transform_edt(~site0, return_indices=True)
            scipy_ms[(H, W, case)] = frame_ms = (time.perf_counter() - t0) * 1e3
            index, dist2 = (t.cpu().numpy() for t in distance.nearest(stack[0], sites))
            yy, xx = np.mgrid[0:H, 0:W]
            assert np.array_equal(np.rint(d ** 2).astype(np.int32), dist2) and (index <= iy * W + ix).all(), case
            assert np.array_equal((index // W - yy) ** 2 + (index % W - xx) ** 2, dist2) and site0.reshape(-1)[index].all(), case
            if case != 'nearest':
                limit = 16 if case == 'grow_r4' else 2 ** 30
                fillv = 255 if case == 'fill_void' else 0
                want = np.where((host[0] == fillv) & (dist2 <= limit), host[0].reshape(-1)[index], host[0])
                assert np.array_equal(fn()[0].cpu().numpy(), want), case
            ms = device_ms(torch, fn, args.warmup, args.iters)
            floor = device_ms(torch, lambda: out32.copy_(stack), args.warmup, args.iters)
            edt = device_ms(torch, lambda: distance.label_edt(mask, 1, out=out32), args.warmup, args.iters)
            res['cases'].append(dict(stack=f'{n}x{H}x{W}', case=case, ms=round(ms, 4), floor_ms=round(floor, 4), label_edt_ms=round(edt, 4),
                                     scipy_frame_ms=round(frame_ms, 2), over_floor=round(ms / floor, 1), over_label_edt=round(ms / edt, 2),
                                     scipy_over_this=round(frame_ms * n / ms, 1), frame_0_checked=True))
            print(json.dumps(res['cases'][-1]), file=sys.stderr, flush=True)
            del stack, mask, out32, out8
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
