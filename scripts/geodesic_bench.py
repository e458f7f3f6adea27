"""Geodesic nearest-site transform measurements (rmem_ocu_amd.distance: geodesic_nearest, geodesic_grow; evaluator.
labels_from_seeds_geodesic, fill_void_geodesic, snap_masks); bench.py is not involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels over synthetic textured RGB frames (a colour per blob of
tests/census_ref.blobs, a slow gradient and +-6 of noise), cases:
  * seeds            20 one-pixel seeds per frame grown into a full label map (labels_from_seeds_geodesic): the long-front case;
  * snap             evaluator.snap_masks(band=3) on the blob annotations displaced by two pixels: the whole call, label_edt and
                     skeleton.thin included;
  * snap_grow        its geodesic_grow alone, on the stack with the band cut out (255);
  * snap_grow_limit  the same with max_cost = 2048;
  * rim              a one-pixel rim of 255 round every blob, filled by fill_void_geodesic.
Weights spatial = 1, colour = 1, batch = 8.  Per case the median ms of `--iters` calls timed one by one with HIP events after
`--warmup` calls, on one stream, with tile skipping on and off (RMEM_GEODESIC_SKIP), the rounds and calls one call takes and the ms
per round, next to three yardsticks from the same run:
  (a) a uint8 -> int32 copy of the stack: the memory floor of a call that writes one map;
  (b) distance.grow on the same labels, fill and sites: the Euclidean twin -- the price of image-awareness;
  (c) scipy.sparse.csgraph.dijkstra(min_only=True) on frame 0's graph on the host (the graph's construction not counted), scaled
      by n; one thread.
Frame 0 of every case is compared with the host first: the cost equals scipy's, the site scipy returns costs the same and never
comes before ours in raster order, and the grown frame equals a gather at our index.
Not measured: the split between begin, rounds and finish, the time the host loop's readbacks leave the device idle, the spread
between runs, other weights or batch sizes.  Prints one JSON line and writes it to --out.
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
CASES = ('seeds', 'snap', 'snap_grow', 'snap_grow_limit', 'rim')
LIMIT = 2048


def make_frames(blobs, seed):
    n, H, W = blobs.shape
    rng = np.random.default_rng(seed)
    table = rng.integers(30, 226, (256, 3))
    y, x = np.mgrid[0:H, 0:W]
    img = table[blobs] + ((x * 24) // W + (y * 16) // H)[None, :, :, None]
    img += rng.integers(-6, 7, img.shape)
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))


def rim_of(a):
    a = a.copy()
    for v in range(1, 11):
        m = a == v
        inner = m.copy()
        inner[:, 1:, :] &= m[:, :-1, :]
        inner[:, :-1, :] &= m[:, 1:, :]
        inner[:, :, 1:] &= m[:, :, :-1]
        inner[:, :, :-1] &= m[:, :, 1:]
        a[m & ~inner] = 255
    return a


def host_graph(image):
    """frame's 8-connected graph as a symmetric sparse matrix of the edge costs at spatial = colour = 1"""
    from scipy.sparse import coo_matrix
    H, W = image.shape[:2]
    im = image.astype(np.int64)
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, vals = [], [], []
    for dy, dx, s in ((0, 1, 5), (1, 0, 5), (1, 1, 7), (1, -1, 7)):
        ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))
        yt, xt = slice(dy, H), slice(max(0, dx), W - max(0, -dx))
        rows.append(idx[ys, xs].reshape(-1))
        cols.append(idx[yt, xt].reshape(-1))
        vals.append((s + np.abs(im[ys, xs] - im[yt, xt]).sum(axis=-1)).reshape(-1))
    return coo_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'geodesic_bench.json'))
    args = ap.parse_args()
    import torch
    from scipy.sparse.csgraph import dijkstra
    from rmem_ocu_amd import distance, skeleton
    from rmem_ocu_amd.evaluator import fill_void_geodesic, labels_from_seeds_geodesic, snap_masks
    dev = torch.device('cuda', 0)
    res = {'metric': 'label_geodesic', 'warmup': args.warmup, 'iters': args.iters, 'host_threads': 1, 'spatial': 1, 'colour': 1, 'batch': 8,
           'tile': list(distance.geodesic_tile()), 'cases': []}
    for n, H, W in STACKS:
        blobs = census_ref.blobs(1000 + H, n, H, W)
        frames = make_frames(blobs, H)
        img = torch.from_numpy(frames).to(dev)
        graph = host_graph(frames[0])
        moved = np.roll(blobs, 2, axis=2)
        for case in CASES:
            limit = LIMIT if case == 'snap_grow_limit' else None
            if case == 'seeds':
                rng = np.random.default_rng(H + W)
                host = np.zeros((n, H, W), dtype=np.uint8)
                for f in range(n):
                    host[f].reshape(-1)[rng.choice(H * W, 20, replace=False)] = np.arange(1, 21, dtype=np.uint8)
                fill = 0
            elif case == 'rim':
                host, fill = rim_of(blobs), 255
            else:
                host, fill = moved, 255
            stack = torch.from_numpy(host).to(dev)
            if case in ('snap_grow', 'snap_grow_limit'):                 # the stack snap_masks grows: the band cut out
                near = (distance.label_edt(stack, border=False) <= 9) & (skeleton.thin(stack) == 0)
                stack = stack.masked_fill(near, 255)
                host = stack.cpu().numpy()
            out32, out8, info = torch.empty(stack.shape, dtype=torch.int32, device=dev), torch.empty_like(stack), {}
            fn = {'seeds': lambda: labels_from_seeds_geodesic(stack, img),
                  'snap': lambda: snap_masks(stack, img, 3),
                  'snap_grow': lambda: distance.geodesic_grow(stack, img, fill=(255,), out=out8, info=info),
                  'snap_grow_limit': lambda: distance.geodesic_grow(stack, img, fill=(255,), max_cost=LIMIT, out=out8, info=info),
                  'rim': lambda: fill_void_geodesic(stack, img)}[case]
            twin = (lambda: distance.grow(stack, fill=(fill,), out=out8)) if case != 'snap' else None
            checked = False
            if case != 'snap':                                           # frame 0 against the host
                sites = np.nonzero(host[0].reshape(-1) != fill)[0]
                t0 = time.perf_counter()
                d, _, src = dijkstra(graph, directed=False, indices=sites, min_only=True, return_predecessors=True)
                frame_ms = (time.perf_counter() - t0) * 1e3
                index, cost = (t.cpu().numpy().reshape(-1) for t in distance.geodesic_nearest(stack[0], img[0], set(range(256)) - {fill}))
                assert np.array_equal(d.astype(np.int64), cost) and (index <= src).all() and (host[0].reshape(-1)[index] != fill).all(), case
                assert np.array_equal(d[index], np.zeros_like(d)) and np.array_equal(cost[src], np.zeros_like(cost)), case
                found = cost <= (LIMIT if limit else 2 ** 30)
                want = np.where((host[0].reshape(-1) == fill) & found, host[0].reshape(-1)[index], host[0].reshape(-1))
                assert np.array_equal(fn()[0].cpu().numpy().reshape(-1), want), case
                checked = True
                distance.geodesic_grow(stack, img, fill=(fill,), max_cost=limit, out=out8, info=info)
            os.environ.pop('RMEM_GEODESIC_SKIP', None)
            ms = device_ms(torch, fn, args.warmup, args.iters)
            os.environ['RMEM_GEODESIC_SKIP'] = '0'
            ms_noskip = device_ms(torch, fn, args.warmup, args.iters)
            os.environ.pop('RMEM_GEODESIC_SKIP', None)
            floor = device_ms(torch, lambda: out32.copy_(stack), args.warmup, args.iters)
            row = dict(stack=f'{n}x{H}x{W}', case=case, ms=round(ms, 3), ms_skip_off=round(ms_noskip, 3), floor_ms=round(floor, 4),
                       over_floor=round(ms / floor, 1), frame_0_checked=checked)
            if twin is not None:
                grow = device_ms(torch, twin, args.warmup, args.iters)
                row.update(rounds=info['rounds'], calls=info['calls'], passes=len(info['passes']), ms_per_round=round(ms / info['rounds'], 4),
                           grow_ms=round(grow, 4), over_grow=round(ms / grow, 1), scipy_frame_ms=round(frame_ms, 1),
                           scipy_over_this=round(frame_ms * n / ms, 1))
            res['cases'].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del stack, out32, out8
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
