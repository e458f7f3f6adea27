"""Surface-metric measurements (rmem_ocu_amd.surface: label_surface, edt_at, surface_census); bench.py is not involved.

Pairs of stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels with 10 objects:
  * blobs   scripts/edt_bench.py's seeded blob annotations against themselves moved by (3, 5);
  * noise   every pixel uniform over 4 values against another draw: every pixel is a surface pixel, every distance is next door --
            the census' heaviest load (64 x 480 x 854 only).
Per case the median ms of `--iters` calls timed one by one with HIP events after `--warmup` calls, on one stream:
  surface_census   the whole call: two surface launches, 2 x 10 sampled transforms, one census;
  its parts        the two surface launches; the 2 x 10 sampled transforms (edt_at); the census alone;
next to yardsticks from the same run:
  (a) distance.hausdorff2 on the same stacks: the set-based number the project already had, 2 x 10 whole-frame transforms and peaks;
  (b) the full-map route to the same table: per object and direction distance.label_edt(surface stack, value=i) into a whole map,
      then a masked copy of the map into the sample stack with torch.where -- what the sampled row pass is meant to save; timed as
      the 2 x 10 transforms with their copies, and as the whole route (surfaces and census included).  The table of route (b) is
      compared with surface_census' table: they must be equal;
  (c) scipy on the host (tests/surface_ref.census) on frame 0, scaled by n; one thread.  surface_census' rows of frame 0 must
      equal it.
Not measured: the split between the column pass and the sampled row pass, the spread between runs.  Prints one JSON line and
writes it to --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import surface_ref as R  # noqa: E402
from edt_bench import device_ms, make_stack  # noqa: E402

CASES = (('blobs', 64, 480, 854), ('blobs', 16, 1080, 1920), ('noise', 64, 480, 854))
K, TOL2, Q = 10, (1, 4), 9500


def make_pair(content, n, H, W):
    a = make_stack(content, n, H, W)
    if content == 'noise':
        return a, np.random.default_rng(H * W).integers(0, 4, (n, H, W)).astype(np.uint8)
    b = np.zeros_like(a)
    b[:, 3:, 5:] = a[:, :-3, :-5]
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'surface_bench.json'))
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import _lib, distance, surface
    L = _lib.lib()
    dev = torch.device('cuda', 0)
    res = {'metric': 'surface_census', 'objects': K, 'tol2': list(TOL2), 'q': Q, 'warmup': args.warmup, 'iters': args.iters,
           'host_threads': 1, 'cases': []}
    for content, n, H, W in CASES:
        ha, hb = make_pair(content, n, H, W)
        a, b = torch.from_numpy(ha).to(dev), torch.from_numpy(hb).to(dev)
        whole = (n * H * W * 11 + int(L.rmem_label_edt_workspace_bytes(n, H, W)) + int(L.rmem_surface_census_workspace_bytes(n, K)))
        stream = torch.cuda.current_stream(dev)
        sa, sb = surface.label_surface(a), surface.label_surface(b)
        da, db = (torch.zeros(a.shape, dtype=torch.int32, device=dev) for _ in range(2))
        dmap = torch.empty(a.shape, dtype=torch.int32, device=dev)
        cws = torch.empty(int(L.rmem_surface_census_workspace_bytes(n, K)), dtype=torch.uint8, device=dev)
        table = torch.empty(n, K, 3, 9, dtype=torch.int64, device=dev)
        tol = (ctypes.c_int * 4)(*TOL2)

        def surfaces():
            surface.label_surface(a)
            surface.label_surface(b)

        def sampled():
            for i in range(1, K + 1):
                surface.edt_at(sb, sa, i, i, da)
                surface.edt_at(sa, sb, i, i, db)

        def full_maps():
            for i in range(1, K + 1):
                distance.label_edt(sb, i, out=dmap)
                torch.where(sa == i, dmap, da, out=da)
                distance.label_edt(sa, i, out=dmap)
                torch.where(sb == i, dmap, db, out=db)

        def census():
            _lib.check(L.rmem_surface_census(da.data_ptr(), sa.data_ptr(), db.data_ptr(), sb.data_ptr(), n, H, W, K, tol, len(TOL2), Q,
                                             table.data_ptr(), cws.data_ptr(), cws.numel(), stream.cuda_stream), 'rmem_surface_census')

        def full_route():
            surfaces()
            full_maps()
            census()

        full_route()
        by_maps = table.clone()
        got = surface.surface_census(a, b, K, TOL2, Q, workspace_bytes=whole)
        assert torch.equal(got, by_maps), (content, n, H, W)
        t0 = time.perf_counter()
        want = R.census(ha[0], hb[0], K, TOL2, Q)
        host_frame_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(got[:1].cpu().numpy(), want), (content, n, H, W)
        ms = {name: device_ms(torch, fn, args.warmup, args.iters) for name, fn in (
            ('surface_census_ms', lambda: surface.surface_census(a, b, K, TOL2, Q, workspace_bytes=whole)),
            ('surfaces_ms', surfaces), ('edt_at_x20_ms', sampled), ('census_ms', census),
            ('hausdorff2_ms', lambda: distance.hausdorff2(a, b, K)),
            ('full_map_x20_ms', full_maps), ('full_map_route_ms', full_route))}
        samples_per_frame = int(want[:, :, 2, 0].sum())
        case = dict(stack=f'{n}x{H}x{W}', content=content, **{k: round(v, 4) for k, v in ms.items()},
                    samples_on_frame_0=samples_per_frame, share_of_frame_0=round(samples_per_frame / (2 * H * W), 4),
                    full_map_over_edt_at=round(ms['full_map_x20_ms'] / ms['edt_at_x20_ms'], 2),
                    full_route_over_surface_census=round(ms['full_map_route_ms'] / ms['surface_census_ms'], 2),
                    hausdorff2_over_surface_census=round(ms['hausdorff2_ms'] / ms['surface_census_ms'], 2),
                    host_frame_ms=round(host_frame_ms, 2), host_over_surface_census=round(host_frame_ms * n / ms['surface_census_ms'], 1),
                    equals_full_map_route=True, equals_host_on_frame_0=True)
        res['cases'].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del a, b, sa, sb, da, db, dmap, cws, table, got, by_maps
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
