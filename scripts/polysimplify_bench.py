"""Ring simplifier measurements (rmem_ocu_amd.polygons: simplify, trace_label_stack(tolerance=...)); bench.py is not involved.

The two 64 x 480 x 854 stacks of scripts/polygons_bench.py (blobs with 10 objects and 0.2 % speckle; noise over 4 values),
8-connectivity, tolerances 0.5, 1 and 2 pixels.  Per content the stack is traced once outside the timed region; per tolerance, ms
per call of polygons.simplify on that table next to two yardsticks of the same run:
  (a) polygons.trace on the same stack, the call it follows;
  (b) a device-to-device rmem_copy_async of the used vertices (8 V bytes), the floor of anything that touches them once.
Every leg takes three readings, the legs alternating; a device reading is the median of `--iters` calls timed one by one with HIP
events after `--warmup` calls.  Also: the vertices kept and the rings left with fewer than 3 vertices per frame, the launches and
the workspace of one call, trace_label_stack on a host clock with and without the tolerance (on the first `--stack-frames-noise`
frames for noise), and as a quality figure the mean J of fill_label_stack(simplified polygons) against the original stack through
evaluator.clip_counts (same frames).  No threshold decides anything here and no host simplifier is installed, so no host speed-up
is claimed; the agreement of frame 0 with tests/polysimplify_ref.py is a check, not a speed comparison.  Prints one JSON line.
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
import polysimplify_ref as S  # noqa: E402
from components_bench import CASE, CONTENTS, device_ms, make_stack  # noqa: E402

NUM_OBJS = {'blobs': 10, 'noise': 3}
CONNECTIVITY = 8
TOLERANCES = (0.5, 1.0, 2.0)
READINGS = 3
LAUNCHES = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=CASE['n'])
    ap.add_argument('--stack-frames-noise', type=int, default=2)
    ap.add_argument('--no-restatement', action='store_true', help='skip the agreement check (the restatement is sequential)')
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import _lib, evaluator, ops, polygons
    dev = torch.device('cuda', 0)
    n, H, W = args.frames, CASE['H'], CASE['W']
    res = {'metric': 'polygon_simplify', 'size': f'{n}x{H}x{W}', 'warmup': args.warmup, 'iters': args.iters, 'readings': READINGS,
           'connectivity': CONNECTIVITY, 'short_max': polygons.short_max(), 'launches': LAUNCHES, 'cases': []}
    stream = torch.cuda.current_stream(dev).cuda_stream
    for content in CONTENTS:
        K = NUM_OBJS[content]
        host = make_stack(content, n, H, W)
        stack = torch.from_numpy(host).to(dev)
        M = polygons.default_max_edges(n, H, W)
        counts = polygons.trace(stack, K, CONNECTIVITY, M)[2].cpu().tolist()
        if counts[3] & polygons.ST_CAPACITY:
            M = counts[0]
        rings, verts, counts_d = polygons.trace(stack, K, CONNECTIVITY, M)
        E, Rn, V, status = counts_d.cpu().tolist()
        assert status == 0
        spare = torch.empty(max(V, 1), 2, dtype=torch.int32, device=dev)
        frames = n if content == 'blobs' else min(n, args.stack_frames_noise)
        part = stack[:frames]
        case = dict(content=content, num_objs=K, max_edges=M, rings_per_frame=round(Rn / n, 1), vertices_per_frame=round(V / n, 1),
                    longest_ring=int(rings[:Rn, 3].max()) if Rn else 0,
                    workspace_MB=round(int(_lib.lib().rmem_polygon_simplify_workspace_bytes(rings.shape[0], verts.shape[0])) / 1e6, 1),
                    trace_label_stack_frames=frames, tolerances=[])

        def stack_route(tol):
            t0 = time.perf_counter()
            out = polygons.trace_label_stack(part, K, CONNECTIVITY, tolerance=tol)
            return (time.perf_counter() - t0) * 1e3, out

        t0_table = None                                             # frame 0 traced by the restatement, once
        for tol in TOLERANCES:
            legs = {
                'simplify_ms': lambda: device_ms(torch, lambda: polygons.simplify(rings, verts, counts_d, tol), args.warmup, args.iters),
                'trace_ms': lambda: device_ms(torch, lambda: polygons.trace(stack, K, CONNECTIVITY, M), args.warmup, args.iters),
                'copy_used_verts_ms': lambda: device_ms(torch, lambda: ops.copy_async(spare, verts, 8 * V)(stream), args.warmup, args.iters),
                'trace_label_stack_ms': lambda: stack_route(None)[0],
                'trace_label_stack_tolerance_ms': lambda: stack_route(tol)[0],
            }
            readings = {k: [] for k in legs}
            for _ in range(READINGS):                               # the legs alternate
                for k, leg in legs.items():
                    readings[k].append(round(leg(), 3))
            med = {k: float(np.median(v)) for k, v in readings.items()}
            rs, vs, cs = polygons.simplify(rings, verts, counts_d, tol)
            c = cs.cpu().tolist()
            few = int((rs[:c[1], 3] < 3).sum())
            polys = polygons.trace_label_stack(part, K, CONNECTIVITY, tolerance=tol)
            back = polygons.fill_label_stack([[(v, p) for v, p in fr.items() if p] for fr in polys], (H, W), dev)
            jc = evaluator.clip_counts(back, part, K + 1)[:, 1:, 4:6].double().cpu().numpy()
            held = jc[..., 1] > 0
            entry = dict(tolerance=tol, status=c[3], vertices_kept_per_frame=round(c[2] / n, 1), kept_share=round(c[2] / max(V, 1), 4),
                         rings_below_3_vertices_per_frame=round(few / n, 1), **{k: round(v, 3) for k, v in med.items()}, readings=readings,
                         simplify_over_trace=round(med['simplify_ms'] / med['trace_ms'], 3),
                         simplify_over_copy=round(med['simplify_ms'] / med['copy_used_verts_ms'], 1),
                         mean_J_of_fill_back=round(float((jc[..., 0][held] / jc[..., 1][held]).mean()), 5) if held.any() else None,
                         changed_pixel_share=round(float((back != torch.where(part > K, torch.zeros_like(part), part)).float().mean()), 6))
            if not args.no_restatement:
                t = t0_table = t0_table if t0_table is not None else R.arrays(host[:1], K, CONNECTIVITY)
                want = S.simplify_arrays(*t, S.steps(tol))
                one = polygons.trace(stack[:1], K, CONNECTIVITY, max(4, int(t[2][0])))
                g = polygons.simplify(*one, tol)
                gc = g[2].cpu().numpy()
                entry['frame0_equals_restatement'] = bool(gc.tolist() == want[2].tolist() and np.array_equal(g[0][:gc[1]].cpu().numpy(), want[0])
                                                          and np.array_equal(g[1][:gc[2]].cpu().numpy(), want[1]))
            case['tolerances'].append(entry)
        res['cases'].append(case)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
