"""Connected-components measurements (rmem_ocu_amd.components: label_components, component_stats, clean_labels); bench.py is not
involved.

One stack of 64 x 480 x 854 uint8 labels in two contents:
  * blobs   seeded blob annotations with 10 objects (tests/census_ref.blobs) and about 0.2 % of the pixels thrown to any of 0..10:
            what a predicted stack looks like before it is cleaned;
  * noise   every pixel uniform over 4 values: nearly every pixel its own piece, the worst case for union-find.
Per content, ms per call of label_components (8-connectivity), of component_stats on its roots and of clean_labels(16, 16,
keep_largest) with its default workspace and status readback, next to two yardsticks on the same stack in the same run:
  (a) a device-to-device rmem_copy_async of the stack's bytes, the floor;
  (b) the host route the feature replaces: stack.cpu(), scipy.ndimage.label per value and frame and the rule in numpy
      (tests/components_ref.clean), and the copy back.  scipy.ndimage.label and the numpy indexing run on one thread however many
      the process may use; the number is in the result.
Every leg takes three readings, the legs alternating; a device reading is the median of `--iters` calls timed one by one with HIP
events after `--warmup` calls, a host reading one pass on a host clock.  The result carries the readings and their median, and
whether clean_labels equals the host route's stack.  Prints one JSON line.
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
import components_ref as R  # noqa: E402

CASE = dict(n=64, H=480, W=854)
CONTENTS = ('blobs', 'noise')
RULE = dict(max_hole_area=16, max_sprinkle_area=16, keep_largest=True, connectivity=8)
READINGS = 3
HOST_THREADS = 1                     # scipy.ndimage.label and numpy fancy indexing are single-threaded


def make_stack(content, n, H, W):
    rng = np.random.default_rng(H + W)
    if content == 'noise':
        return rng.integers(0, 4, (n, H, W)).astype(np.uint8)
    a = census_ref.blobs(1000 + H, n, H, W)
    hit = rng.random((n, H, W)) < 0.002
    a[hit] = rng.integers(0, 11, (n, H, W)).astype(np.uint8)[hit]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import components, ops
    dev = torch.device('cuda', 0)
    n, H, W = CASE['n'], CASE['H'], CASE['W']
    nbytes = n * H * W
    res = {'metric': 'label_components', 'size': f'{n}x{H}x{W}', 'label_MB': round(nbytes / 1e6, 2), 'warmup': args.warmup,
           'iters': args.iters, 'readings': READINGS, 'rule': RULE, 'tile': list(components.tile()), 'host_threads': HOST_THREADS,
           'cases': []}
    for content in CONTENTS:
        stack = torch.from_numpy(make_stack(content, n, H, W)).to(dev)
        out = torch.empty_like(stack)
        stream = torch.cuda.current_stream(dev).cuda_stream
        roots, status = components.label_components(stack, RULE['connectivity'])
        host_result = {}

        def host_route():
            t0 = time.perf_counter()
            host = stack.cpu().numpy()
            cleaned = R.clean(host, RULE['max_hole_area'], RULE['max_sprinkle_area'], RULE['keep_largest'], RULE['connectivity'])
            back = torch.from_numpy(cleaned).to(dev)
            torch.cuda.synchronize()
            host_result['stack'] = back
            return (time.perf_counter() - t0) * 1e3

        legs = {
            'components_ms': lambda: device_ms(torch, lambda: components.label_components(stack, RULE['connectivity']), args.warmup, args.iters),
            'stats_ms': lambda: device_ms(torch, lambda: components.component_stats(stack, roots, RULE['connectivity']), args.warmup, args.iters),
            'clean_ms': lambda: device_ms(torch, lambda: components.clean_labels(stack, out=out, **RULE), args.warmup, args.iters),
            'copy_ms': lambda: device_ms(torch, lambda: ops.copy_async(out, stack, nbytes)(stream), args.warmup, args.iters),
            'host_route_ms': host_route,
        }
        readings = {k: [] for k in legs}
        for _ in range(READINGS):                                   # the legs alternate
            for k, leg in legs.items():
                readings[k].append(round(leg(), 3))
        cleaned = components.clean_labels(stack, **RULE)
        med = {k: float(np.median(v)) for k, v in readings.items()}
        _, table = components.component_stats(stack, roots, RULE['connectivity'])
        res['cases'].append(dict(content=content, pieces_per_frame=round(float(table[:, :, 0].sum().item()) / n, 1),
                                 status=int(status.item()), **{k: round(v, 3) for k, v in med.items()}, readings=readings,
                                 clean_over_copy=round(med['clean_ms'] / med['copy_ms'], 1),
                                 host_over_clean=round(med['host_route_ms'] / med['clean_ms'], 1),
                                 clean_equals_host_route=bool(torch.equal(cleaned, host_result['stack']))))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
