"""Polygon fill measurements (rmem_ocu_amd.polygons: PackedPolygons, fill_labels_into); bench.py is not involved.

The blob stack of scripts/components_bench.py and polygons_bench.py: 64 x 480 x 854 uint8 labels, seeded blob annotations with 10
objects (tests/census_ref.blobs) and about 0.2 % of the pixels thrown to any of 0..10.  Its polygons come from
polygons.trace_label_stack (8-connectivity), outside every timed region; one shape per frame and object, every speck a ring.
ms per call of polygons.fill_labels_into from a ready PackedPolygons (the copy of the pack from pinned memory included), next to
three yardsticks on the same stack in the same run:
  (a) a device-to-device rmem_copy_async of the stack's bytes, the floor of anything that writes the stack;
  (b) rle.decode_labels_into of the same stack's run-length strings, the sibling input format;
  (c) a host-to-device copy of the finished stack from pinned memory, the least a host rasteriser would still pay.
Every leg takes three readings, the legs alternating; a reading is the median of `--iters` calls timed one by one with HIP events
after `--warmup` calls.  PackedPolygons(...) is timed on a host clock, separately, three times.  The result carries every
reading, the edges, crossings, plane bytes and launches of one call, and whether the filled stack equals the traced one and frame 0
the sequential restatement's (tests/polyfill_ref.py) -- agreement checks, not speed comparisons.  No host rasteriser is timed, so
no speed-up over one is claimed.  Writes one JSON line to `--out` and prints it.
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

import polyfill_ref as P  # noqa: E402
from components_bench import CASE, device_ms, make_stack  # noqa: E402

NUM_OBJS = 10
CONNECTIVITY = 8
READINGS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=CASE['n'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'polyfill_bench.json'))
    ap.add_argument('--no-restatement', action='store_true', help='skip the agreement check of frame 0 (the restatement is sequential)')
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import ops, polygons, rle
    dev = torch.device('cuda', 0)
    n, H, W = args.frames, CASE['H'], CASE['W']
    nbytes = n * H * W
    host = make_stack('blobs', n, H, W)
    stack = torch.from_numpy(host).to(dev)
    out = torch.empty_like(stack)
    pinned = torch.from_numpy(host).pin_memory()
    stream = torch.cuda.current_stream(dev).cuda_stream

    frames = polygons.trace_label_stack(stack, NUM_OBJS, CONNECTIVITY)           # outside every timed region
    pack_ms = []
    for _ in range(READINGS):
        t0 = time.perf_counter()
        packed = polygons.PackedPolygons(frames, (H, W))
        pack_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
    strings = rle.PackedRles(rle.encode_label_stack(stack, NUM_OBJS), (H, W))

    legs = {
        'fill_ms': lambda: device_ms(torch, lambda: polygons.fill_labels_into(packed, out), args.warmup, args.iters),
        'copy_ms': lambda: device_ms(torch, lambda: ops.copy_async(out, stack, nbytes)(stream), args.warmup, args.iters),
        'rle_decode_ms': lambda: device_ms(torch, lambda: rle.decode_labels_into(strings, out), args.warmup, args.iters),
        'pinned_upload_ms': lambda: device_ms(torch, lambda: out.copy_(pinned, non_blocking=True), args.warmup, args.iters),
    }
    readings = {k: [] for k in legs}
    for _ in range(READINGS):                                       # the legs alternate
        for k, leg in legs.items():
            readings[k].append(round(leg(), 3))
    med = {k: float(np.median(v)) for k, v in readings.items()}

    out.fill_(0xA5)
    polygons.fill_labels_into(packed, out)
    packed.check(dev)
    got = out.cpu().numpy()
    passes = packed.passes()
    res = dict(metric='polygon_fill', size=f'{n}x{H}x{W}', label_MB=round(nbytes / 1e6, 2), content='blobs, 10 objects, 0.2 % speckle',
               connectivity=CONNECTIVITY, warmup=args.warmup, iters=args.iters, readings_per_leg=READINGS,
               shapes=packed.nshapes, rings=int(sum(len(p['holes']) + 1 for fr in frames for polys in fr.values() for p in polys)),
               edges=packed.nedges, crossings=packed.crossings, pack_KB=round((packed.buf.numel() + packed.desc_bytes.numel()) / 1e3, 1),
               plane_MB=round(4 * packed.plane_words / 1e6, 2), passes=len(passes), launches=1 + 5 * len(passes),
               **{k: round(v, 3) for k, v in med.items()}, readings=readings, pack_host_ms=pack_ms,
               fill_over_copy=round(med['fill_ms'] / med['copy_ms'], 1), fill_over_rle_decode=round(med['fill_ms'] / med['rle_decode_ms'], 2),
               fill_over_pinned_upload=round(med['fill_ms'] / med['pinned_upload_ms'], 2),
               filled_equals_traced_stack=bool(np.array_equal(got, host)),
               not_measured='other sizes, noise content, a host rasteriser (Pillow, pycocotools)')
    if not args.no_restatement:
        want = P.paint_stack([[(v, [p['exterior']] + p['holes']) for v, polys in frames[0].items() for p in polys]], H, W)
        res['frame0_equals_restatement'] = bool(np.array_equal(got[0], want[0]))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
