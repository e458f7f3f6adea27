"""Polygon tracer measurements (rmem_ocu_amd.polygons: trace, trace_label_stack); bench.py is not involved.

The stack of scripts/components_bench.py, 64 x 480 x 854 uint8 labels in two contents:
  * blobs   seeded blob annotations with 10 objects (tests/census_ref.blobs) and about 0.2 % of the pixels thrown to any of 0..10;
  * noise   every pixel uniform over 4 values (3 objects): about three edges per object pixel and rings of a few edges, the most
            rings and vertices a stack can have short of a checkerboard.
Per content, ms per call of polygons.trace (8-connectivity; max_edges = default_max_edges where the edges fit it, else the exact
count a first call reported) and of trace_label_stack end to end, readbacks and the grouping in Python included (on the first
`--stack-frames-noise` frames for noise, whose hundreds of thousands of rings per frame the grouping walks one by one), next to
three yardsticks on the same stack in the same run:
  (a) a device-to-device rmem_copy_async of the stack's bytes, the floor;
  (b) rle.encode of the same stack, the sibling output format, also built on the device;
  (c) components.clean_labels(16, 16, keep_largest).
Every leg takes three readings, the legs alternating; a device reading is the median of `--iters` calls timed one by one with HIP
events after `--warmup` calls, trace_label_stack one pass on a host clock.  The result carries the readings and their median, E,
R and V per frame, the launches of one call, and whether the device's rings of frame 0 equal the sequential restatement's
(tests/polygons_ref.py) -- an agreement check, not a speed comparison.  Prints one JSON line.
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
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import polygons_ref as R  # noqa: E402
from components_bench import CASE, CONTENTS, RULE, device_ms, make_stack  # noqa: E402

NUM_OBJS = {'blobs': 10, 'noise': 3}
CONNECTIVITY = 8
READINGS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=CASE['n'])
    ap.add_argument('--stack-frames-noise', type=int, default=2)
    ap.add_argument('--no-restatement', action='store_true', help='skip the agreement check (the restatement is sequential)')
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import _lib, components, ops, polygons, rle
    dev = torch.device('cuda', 0)
    n, H, W = args.frames, CASE['H'], CASE['W']
    nbytes = n * H * W
    res = {'metric': 'label_polygons', 'size': f'{n}x{H}x{W}', 'label_MB': round(nbytes / 1e6, 2), 'warmup': args.warmup,
           'iters': args.iters, 'readings': READINGS, 'connectivity': CONNECTIVITY, 'unit': polygons.unit(), 'cases': []}
    for content in CONTENTS:
        K = NUM_OBJS[content]
        host = make_stack(content, n, H, W)
        stack = torch.from_numpy(host).to(dev)
        out = torch.empty_like(stack)
        stream = torch.cuda.current_stream(dev).cuda_stream
        M = polygons.default_max_edges(n, H, W)
        counts = polygons.trace(stack, K, CONNECTIVITY, M)[2].cpu().tolist()
        fits = not counts[3] & polygons.ST_CAPACITY
        if not fits:
            M = counts[0]
            counts = polygons.trace(stack, K, CONNECTIVITY, M)[2].cpu().tolist()
        stack_frames = n if content == 'blobs' else min(n, args.stack_frames_noise)

        def stack_route():
            t0 = time.perf_counter()
            polygons.trace_label_stack(stack[:stack_frames], K, CONNECTIVITY)
            return (time.perf_counter() - t0) * 1e3

        legs = {
            'trace_ms': lambda: device_ms(torch, lambda: polygons.trace(stack, K, CONNECTIVITY, M), args.warmup, args.iters),
            'copy_ms': lambda: device_ms(torch, lambda: ops.copy_async(out, stack, nbytes)(stream), args.warmup, args.iters),
            'rle_ms': lambda: device_ms(torch, lambda: rle.encode(stack, K), args.warmup, args.iters),
            'clean_ms': lambda: device_ms(torch, lambda: components.clean_labels(stack, out=out, **RULE), args.warmup, args.iters),
            'trace_label_stack_ms': stack_route,
        }
        readings = {k: [] for k in legs}
        for _ in range(READINGS):                                   # the legs alternate
            for k, leg in legs.items():
                readings[k].append(round(leg(), 3))
        med = {k: float(np.median(v)) for k, v in readings.items()}
        rounds = int(np.ceil(np.log2(min(M, 4 * H * W))))
        case = dict(content=content, num_objs=K, max_edges=M, default_max_edges_fits=fits, status=counts[3],
                    edges_per_frame=round(counts[0] / n, 1), rings_per_frame=round(counts[1] / n, 1),
                    vertices_per_frame=round(counts[2] / n, 1), launches=15 + rounds,
                    workspace_MB=round(int(_lib.lib().rmem_label_polygons_workspace_bytes(n, H, W, M)) / 1e6, 1),
                    trace_label_stack_frames=stack_frames, **{k: round(v, 3) for k, v in med.items()}, readings=readings,
                    trace_over_copy=round(med['trace_ms'] / med['copy_ms'], 1), trace_over_rle=round(med['trace_ms'] / med['rle_ms'], 2),
                    trace_over_clean=round(med['trace_ms'] / med['clean_ms'], 2))
        if not args.no_restatement:
            want = R.arrays(host[:1], K, CONNECTIVITY)
            rings, verts, c = polygons.trace(stack[:1], K, CONNECTIVITY, max(4, int(want[2][0])))
            c = c.cpu().numpy()
            case['frame0_equals_restatement'] = bool(c.tolist() == want[2].tolist() and np.array_equal(rings[:c[1]].cpu().numpy(), want[0])
                                                     and np.array_equal(verts[:c[2]].cpu().numpy(), want[1]))
        res['cases'].append(case)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
