"""Stroke rasteriser measurements (rmem_ocu_amd.strokes: PackedStrokes, draw_labels_into); bench.py is not involved.

A 64 x 480 x 854 uint8 stack with 10 seeded random-walk strokes of 40 vertices per frame (steps of up to 12 pixels, values 1..10),
drawn at r = 0 (hairlines) and r = 3 (a round brush), with every frame stroked into a fresh stack, and with ONE frame stroked in
`over` mode onto an existing stack -- the interactive case.  ms per call of strokes.draw_labels_into from a ready PackedStrokes
(the copy of the pack from pinned memory included), next to three yardsticks in the same run:
  (a) a device-to-device rmem_copy_async of the stack's bytes, the floor of anything that writes the stack;
  (b) polygons.fill_labels_into on the blob stack of scripts/polyfill_bench.py, the sibling rasteriser;
  (c) a host-to-device copy of the finished stack from pinned memory, the least a host rasteriser would still pay.
Every leg takes three readings, the legs alternating; a reading is the median of `--iters` calls timed one by one with HIP events
after `--warmup` calls.  PackedStrokes(...) is timed on a host clock, separately, three times per radius.  The result carries every
reading, the segments, work items, owner-map bytes and launches of one call, and whether frame 0 equals the sequential
restatement's (tests/strokes_ref.py) and the `over` call changed the stroked frame alone -- agreement checks, not speed
comparisons.  No host rasteriser is timed, so no speed-up over one is claimed.  Writes one JSON line to `--out` and prints it.
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

import strokes_ref as S  # noqa: E402
from components_bench import CASE, device_ms, make_stack  # noqa: E402

NUM_OBJS = 10
VERTICES = 40
STEP = 12.0
READINGS = 3
SEED = 20240


def make_strokes(n, H, W, radius):
    rng = np.random.default_rng(SEED)
    return [[{'value': 1 + k, 'path': S.random_walk(rng, H, W, VERTICES, step=STEP), 'radius': radius} for k in range(NUM_OBJS)] for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=CASE['n'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'strokes_bench.json'))
    ap.add_argument('--no-restatement', action='store_true', help='skip the agreement check of frame 0 (the restatement is sequential)')
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import ops, polygons, strokes
    dev = torch.device('cuda', 0)
    n, H, W = args.frames, CASE['H'], CASE['W']
    nbytes = n * H * W
    host = make_stack('blobs', n, H, W)
    stack = torch.from_numpy(host).to(dev)
    out = torch.empty_like(stack)
    pinned = torch.from_numpy(host).pin_memory()
    stream = torch.cuda.current_stream(dev).cuda_stream
    polys = polygons.PackedPolygons(polygons.trace_label_stack(stack, NUM_OBJS, 8), (H, W))     # outside every timed region

    packs, pack_ms, lists = {}, {}, {}
    mid = n // 2
    for r in (0, 3):
        lists[r] = make_strokes(n, H, W, r)
        pack_ms[f'r{r}'] = []
        for _ in range(READINGS):
            t0 = time.perf_counter()
            packs[r, 'all'] = strokes.PackedStrokes(lists[r], (H, W))
            pack_ms[f'r{r}'].append(round((time.perf_counter() - t0) * 1e3, 1))
        packs[r, 'one'] = strokes.PackedStrokes([fr if f == mid else [] for f, fr in enumerate(lists[r])], (H, W))

    def draw(r, which, over):
        return lambda: device_ms(torch, lambda: strokes.draw_labels_into(packs[r, which], out, over=over), args.warmup, args.iters)

    legs = {
        'draw_r0_all_ms': draw(0, 'all', False), 'draw_r3_all_ms': draw(3, 'all', False),
        'draw_r0_one_over_ms': draw(0, 'one', True), 'draw_r3_one_over_ms': draw(3, 'one', True),
        'copy_ms': lambda: device_ms(torch, lambda: ops.copy_async(out, stack, nbytes)(stream), args.warmup, args.iters),
        'polygon_fill_ms': lambda: device_ms(torch, lambda: polygons.fill_labels_into(polys, out), args.warmup, args.iters),
        'pinned_upload_ms': lambda: device_ms(torch, lambda: out.copy_(pinned, non_blocking=True), args.warmup, args.iters),
    }
    readings = {k: [] for k in legs}
    for _ in range(READINGS):                                       # the legs alternate
        for k, leg in legs.items():
            readings[k].append(round(leg(), 3))
    med = {k: float(np.median(v)) for k, v in readings.items()}

    res = dict(metric='stroke_draw', size=f'{n}x{H}x{W}', label_MB=round(nbytes / 1e6, 2),
               content=f'{NUM_OBJS} random-walk strokes of {VERTICES} vertices per frame, steps up to {STEP} px, seed {SEED}',
               warmup=args.warmup, iters=args.iters, readings_per_leg=READINGS, **{k: round(v, 3) for k, v in med.items()},
               readings=readings, pack_host_ms=pack_ms)
    for r in (0, 3):
        for which in ('all', 'one'):
            p = packs[r, which]
            passes = p.passes()
            res[f'r{r}_{which}'] = dict(strokes=p.nstrokes, segments=p.nsegs, items=p.items, stroked_frames=len(p.stroked),
                                        pack_KB=round((p.buf.numel() + p.desc_bytes.numel()) / 1e3, 1),
                                        owner_MB=round(4 * len(p.stroked) * H * W / 1e6, 2), passes=len(passes), launches=1 + 5 * len(passes))
        out.fill_(0xA5)
        strokes.draw_labels_into(packs[r, 'all'], out)
        packs[r, 'all'].check(dev)
        got = out.cpu().numpy()
        res[f'r{r}_covered_fraction'] = round(float((got != 0).mean()), 5)
        if not args.no_restatement:
            want = np.zeros((H, W), dtype=np.uint8)
            for s in lists[r][0]:
                pts = S.points(s['path'])
                mask = S.brush_mask_large(pts, S.quantise(r), H, W) if r else S.mask_of(S.hairline_pixels(pts, H, W), H, W)
                want[mask] = s['value']
            res[f'r{r}_frame0_equals_restatement'] = bool(np.array_equal(got[0], want))
        out.copy_(stack)
        strokes.draw_labels_into(packs[r, 'one'], out, over=True)
        packs[r, 'one'].check(dev)
        over = out.cpu().numpy()
        changed = np.flatnonzero((over != host).reshape(n, -1).any(axis=1)).tolist()
        res[f'r{r}_over_changed_frames'] = changed
        res[f'r{r}_over_equals_fresh_where_covered'] = bool(np.array_equal(over[mid][got[mid] != 0], got[mid][got[mid] != 0])
                                                            and np.array_equal(over[mid][got[mid] == 0], host[mid][got[mid] == 0]))
    res['not_measured'] = 'other sizes, radii and stroke counts, strokes of few long segments, a host rasteriser (Pillow, OpenCV)'
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
