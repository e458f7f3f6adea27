"""Label census / remap measurements (rmem_label_census, rmem_label_remap through rmem_ocu_amd.protocol); bench.py is not involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels, three contents each:
  * blobs       seeded blob annotations with 10 objects (tests/census_ref.blobs);
  * background  all zero: every wave of every workgroup meets on label 0 (worst contention);
  * noise       every pixel uniform over 11 ids: every lane's 16 bytes are mixed and every wave holds all 11 (worst divergence).
Per stack: us per call and GB/s of label bytes, the median of `--iters` calls timed one by one with HIP events on one stream after
`--warmup` calls, for the census and for the remap (one table per frame, out of place), and two yardsticks on the same stack in
the same run: a device-to-device rmem_copy_async of the same bytes, and the host route the census replaces -- stack.cpu(), then
per frame np.bincount and numpy boxes (median of `--cpu-rounds` passes on a host clock).  Whether the census equals the host
route's numbers is reported too.  Prints one JSON line.
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

import census_ref as R  # noqa: E402

CASES = (dict(n=64, H=480, W=854), dict(n=16, H=1080, W=1920))
CONTENTS = ('blobs', 'background', 'noise')


def make_stack(content, n, H, W):
    if content == 'blobs':
        return R.blobs(1000 + H, n, H, W)
    if content == 'background':
        return np.zeros((n, H, W), dtype=np.uint8)
    return np.random.default_rng(H).integers(0, 11, (n, H, W)).astype(np.uint8)


def host_census(stack_d):
    """the route the device census replaces: the stack over PCIe, np.bincount and numpy boxes per frame"""
    stack = stack_d.cpu().numpy()
    n, H, W = stack.shape
    out = np.empty((n, 256, 5), dtype=np.int32)
    out[:] = (0, W, H, -1, -1)
    for f in range(n):
        area = np.bincount(stack[f].reshape(-1), minlength=256)
        for v in np.nonzero(area)[0]:
            m = stack[f] == v
            ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
            out[f, v] = (area[v], xs[0], ys[0], xs[-1], ys[-1])
    return out


def device_us(torch, fn, warmup, iters):
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
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--cpu-rounds', type=int, default=3)
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.protocol import label_census, remap_labels
    dev = torch.device('cuda', 0)
    res = {'metric': 'label_census', 'warmup': args.warmup, 'iters': args.iters, 'cases': []}
    for c in CASES:
        n, H, W = c['n'], c['H'], c['W']
        nbytes = n * H * W
        luts = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (n, 256)).astype(np.uint8)).to(dev)
        for content in CONTENTS:
            stack = torch.from_numpy(make_stack(content, n, H, W)).to(dev)
            out = torch.empty_like(stack)
            stream = torch.cuda.current_stream(dev).cuda_stream
            census_us = device_us(torch, lambda: label_census(stack), args.warmup, args.iters)
            remap_us = device_us(torch, lambda: remap_labels(stack, luts, out=out), args.warmup, args.iters)
            copy_us = device_us(torch, lambda: ops.copy_async(out, stack, nbytes)(stream), args.warmup, args.iters)
            host, want = [], None
            for _ in range(args.cpu_rounds):
                t0 = time.perf_counter()
                want = host_census(stack)
                host.append((time.perf_counter() - t0) * 1e6)
            area, box = label_census(stack)
            equal = bool(np.array_equal(area.cpu().numpy(), want[:, :, 0]) and np.array_equal(box.cpu().numpy(), want[:, :, 1:]))

            def gbs(us):
                return round(nbytes / us / 1e3, 1)

            host_us = float(np.median(host))
            res['cases'].append(dict(size=f'{n}x{H}x{W}', content=content, label_MB=round(nbytes / 1e6, 2),
                                     census_us=round(census_us, 1), census_GB_per_s=gbs(census_us),
                                     remap_us=round(remap_us, 1), remap_GB_per_s=gbs(remap_us),
                                     copy_us=round(copy_us, 1), copy_GB_per_s=gbs(copy_us),
                                     host_route_us=round(host_us, 1), host_route_GB_per_s=gbs(host_us),
                                     census_over_copy=round(census_us / copy_us, 2), host_over_census=round(host_us / census_us, 1),
                                     census_equals_host_route=equal))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
