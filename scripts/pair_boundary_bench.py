"""Pair boundary census measurements (rmem_pair_boundary_counts through rmem_ocu_amd.pairs.pair_boundary_counts); bench.py is not
involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels (a against b), the default bound_th of 0.008 (radius 8 and 18):
  * blobs, num = 10   seeded blob annotations with 10 objects (tests/census_ref.blobs) against the same blobs moved by (2, 3)
                      pixels: what a prediction against its annotation looks like;
  * blobs, num = 40   the same with 40 objects: beyond the diagonal scorer's 31;
  * cells, num = 255  a 16 x 16 grid of cells, each holding one small object (a third of the cell each way), ids 1..255, against
                      the same moved by (3, 5) pixels; void_label None.
Per case: us per call, the median of `--iters` calls timed one by one with HIP events on one stream after `--warmup` calls, the
frames per pass of the default workspace, and two yardsticks on the same stacks in the same run, because no earlier commit has
this route:
  (a) diagonal  evaluator.clip_counts (rmem_clip_score_counts, id i against id i only) at 10 objects -- the route the parent commit
                has, its code untouched; pair / diagonal is reported, and whether the pair table's diagonal equals its counts;
  (b) host      .cpu() of both stacks plus the numpy / scipy restatement (tests/pair_boundary_ref.py) on the first frame, for the
                num = 10 cases (the restatement's matrices of 255 ids x 2 M pixels do not fit a host); reported per frame and
                scaled to the stack by n, and whether the device tables of that frame equal it.
Writes one JSON document to --out and prints it.
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
import pair_boundary_ref  # noqa: E402

CASES = (dict(n=64, H=480, W=854), dict(n=16, H=1080, W=1920))
CONTENTS = (('blobs', 10), ('blobs', 40), ('cells', 255))
HOST_FRAMES = 1


def make_stacks(content, num, n, H, W):
    if content == 'blobs':
        a = census_ref.blobs(1000 + H + num, n, H, W, ids=tuple(range(1, num + 1)))
        return a, np.roll(a, (2, 3), axis=(1, 2))
    ch, cw = H // 16, W // 16
    frame = np.zeros((H, W), dtype=np.uint8)
    for v in range(1, 256):
        y, x = (v // 16) * ch + ch // 3, (v % 16) * cw + cw // 3
        frame[y:y + ch // 3, x:x + cw // 3] = v
    a = np.ascontiguousarray(np.broadcast_to(frame, (n, H, W)))
    return a, np.roll(a, (3, 5), axis=(1, 2))


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
    ap.add_argument('--cases', type=int, default=len(CASES), help='the first CASES only (a rehearsal)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pair_boundary_bench.json'))
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import _lib, pairs
    from rmem_ocu_amd.evaluator import boundary_radius, clip_counts
    if not torch.cuda.is_available():
        raise SystemExit('pair_boundary_bench: no GPU')
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    res = {'metric': 'pair_boundary_counts', 'warmup': args.warmup, 'iters': args.iters, 'bound_th': 0.008,
           'workspace_cap_MiB': pairs.PAIR_BOUNDARY_WORKSPACE_CAP >> 20, 'host_frames': HOST_FRAMES, 'cases': []}
    for c in CASES[:args.cases]:
        n, H, W = c['n'], c['H'], c['W']
        diagonal_us = None
        for content, num in CONTENTS:
            a_h, b_h = make_stacks(content, num, n, H, W)
            a, b = torch.from_numpy(a_h).to(dev), torch.from_numpy(b_h).to(dev)
            void = None if num == 255 else 255
            per_frame = L.rmem_pair_boundary_workspace_bytes(1, H, W, num, num)
            row = dict(size=f'{n}x{H}x{W}', content=content, num=num, radius=boundary_radius(H, W),
                       planes_MB_per_frame=round(per_frame / 1e6, 2),
                       frames_per_pass=int(min(n, max(1, pairs.PAIR_BOUNDARY_WORKSPACE_CAP // per_frame))))
            pair_us = device_us(torch, lambda: pairs.pair_boundary_counts(a, b, num, num, void), args.warmup, args.iters)
            row.update(pair_us=round(pair_us, 1), pair_us_per_frame=round(pair_us / n, 1))
            match, bnd_a, bnd_b = (t.cpu().numpy() for t in pairs.pair_boundary_counts(a, b, num, num, void))
            row['nonzero_pairs_per_frame'] = round(float(match.any(axis=3).sum()) / n, 1)
            if num == 10:
                diagonal_us = device_us(torch, lambda: clip_counts(a, b, num + 1), args.warmup, args.iters)
                counts = clip_counts(a, b, num + 1).cpu().numpy()
                d = np.arange(num + 1)
                row['diagonal_equals_clip_counts'] = bool(
                    np.array_equal(bnd_a, counts[:, :, 0]) and np.array_equal(bnd_b, counts[:, :, 1]) and
                    np.array_equal(match[:, d, d, 0], counts[:, :, 2]) and np.array_equal(match[:, d, d, 1], counts[:, :, 3]))
                t0 = time.perf_counter()
                want = pair_boundary_ref.tables(a[:HOST_FRAMES].cpu().numpy(), b[:HOST_FRAMES].cpu().numpy(), num, num, void)
                host_us = (time.perf_counter() - t0) * 1e6 * n / HOST_FRAMES
                row.update(host_us_scaled=round(host_us, 1), host_over_pair=round(host_us / pair_us, 1),
                           equals_host_restatement=bool(all(np.array_equal(g[:HOST_FRAMES], w)
                                                            for g, w in zip((match, bnd_a, bnd_b), want))))
            row.update(diagonal10_us=round(diagonal_us, 1), pair_over_diagonal10=round(pair_us / diagonal_us, 2))
            res['cases'].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
