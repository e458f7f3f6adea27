"""Label-tube measurements (rmem_ocu_amd.tubes: label_tubes, lineage, piece_events, tube_table, clean_tubes); bench.py is not
involved.

Two stacks of uint8 labels, 64 x 480 x 854 and 16 x 1080 x 1920: seeded blob annotations with 10 objects drifting by (1, 2) pixels
per frame and 2-frame specks (tests/tubes_ref.content 'drift').  Per stack, ms per call on one MI355X and one stream of
  * tubes_ms            rmem_label_tubes alone, given the roots (8-connectivity, temporal = 1);
  * lineage_events_ms   rmem_label_tube_lineage + rmem_label_tube_events;
  * index_table_ms      rmem_label_tube_index + rmem_label_tube_table (rows = the number of tubes);
  * clean_tubes_ms      tubes.clean_tubes(min_frames=3, max_hole_frames=2) whole: components, statistics, tubes, index, the
                        8-byte readback, table, clean;
next to three yardsticks from the same run:
  * copy_ms             a uint8 -> int32 copy of the stack (the floor of any pass that writes one int per voxel);
  * clean_labels_ms     components.clean_labels(16, 16, keep_largest) on the same stack: the per-frame clean-up;
  * scipy_label_ms      scipy.ndimage.label with the 3-D structure, value by value, on one host thread (one pass on a host clock).
A device number is the median of `--iters` calls timed one by one with HIP events after `--warmup` calls.  Writes the result to
`--out` (profiles/tubes_bench.json) and prints it as one JSON line.
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

import tubes_ref as R  # noqa: E402

CASES = (dict(n=64, H=480, W=854), dict(n=16, H=1080, W=1920))
CONN, TEMPORAL = 8, 1
RULE = dict(min_frames=3, max_hole_frames=2)
HOST_THREADS = 1                     # scipy.ndimage.label is single-threaded


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
    return round(float(np.median(times)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tubes_bench.json'))
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    from rmem_ocu_amd import _lib, components, tubes
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    res = {'metric': 'label_tubes', 'connectivity': CONN, 'temporal': TEMPORAL, 'rule': RULE, 'warmup': args.warmup, 'iters': args.iters,
           'host_threads': HOST_THREADS, 'cases': []}
    for case in CASES:
        n, H, W = case['n'], case['H'], case['W']
        host = R.content('drift', n, H, W)
        stack = torch.from_numpy(host.copy()).to(dev)
        out, wide = torch.empty_like(stack), torch.empty(stack.shape, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        s = stream.cuda_stream
        roots, status = components.label_components(stack, CONN)
        stats, _ = components.component_stats(stack, roots, CONN)
        t = tubes._tubes(stack, roots, TEMPORAL, status, stream)
        links = tubes._links(stack, roots, TEMPORAL, stream)
        events = torch.empty(n, 256, 4, dtype=torch.int32, device=dev)
        rank, total = tubes._index(stack, t, stream)
        T = int(total.item())
        table = torch.empty(T, 10, dtype=torch.int32, device=dev)
        p = stack.data_ptr()

        def do_tubes():
            _lib.check(L.rmem_label_tubes(p, roots.data_ptr(), n, H, W, TEMPORAL, t.data_ptr(), status.data_ptr(), s), 'rmem_label_tubes')

        def do_lineage_events():
            _lib.check(L.rmem_label_tube_lineage(p, roots.data_ptr(), n, H, W, TEMPORAL, links.data_ptr(), s), 'rmem_label_tube_lineage')
            _lib.check(L.rmem_label_tube_events(p, roots.data_ptr(), links.data_ptr(), n, H, W, events.data_ptr(), s), 'rmem_label_tube_events')

        def do_index_table():
            _lib.check(L.rmem_label_tube_index(t.data_ptr(), n, H, W, rank.data_ptr(), total.data_ptr(), s), 'rmem_label_tube_index')
            _lib.check(L.rmem_label_tube_table(p, roots.data_ptr(), stats.data_ptr(), t.data_ptr(), rank.data_ptr(), n, H, W, T,
                                               table.data_ptr(), s), 'rmem_label_tube_table')

        row = dict(size=f'{n}x{H}x{W}', label_MB=round(n * H * W / 1e6, 2), tubes=T)
        row['tubes_ms'] = device_ms(torch, do_tubes, args.warmup, args.iters)
        row['lineage_events_ms'] = device_ms(torch, do_lineage_events, args.warmup, args.iters)
        row['index_table_ms'] = device_ms(torch, do_index_table, args.warmup, args.iters)
        row['clean_tubes_ms'] = device_ms(torch, lambda: tubes.clean_tubes(stack, connectivity=CONN, temporal=TEMPORAL, out=out, **RULE),
                                          args.warmup, args.iters)
        row['copy_ms'] = device_ms(torch, lambda: wide.copy_(stack), args.warmup, args.iters)
        row['clean_labels_ms'] = device_ms(torch, lambda: components.clean_labels(stack, 16, 16, True, CONN, out=out), args.warmup, args.iters)
        t0 = time.perf_counter()
        pieces = 0
        for v in np.unique(host):
            pieces += ndimage.label(host == v, structure=R.structure(CONN, TEMPORAL))[1]
        row['scipy_label_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        cleaned = tubes.clean_tubes(stack, connectivity=CONN, temporal=TEMPORAL, **RULE)
        row['status'] = int(status.item())
        row['scipy_tubes'] = int(pieces)
        row['voxels_changed'] = int((cleaned != stack).sum().item())
        row['tubes_over_copy'] = round(row['tubes_ms'] / row['copy_ms'], 1)
        row['clean_tubes_over_clean_labels'] = round(row['clean_tubes_ms'] / row['clean_labels_ms'], 2)
        res['cases'].append(row)
        del stack, out, wide, roots, stats, t, links, events, rank, table, cleaned
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text, flush=True)


if __name__ == '__main__':
    main()
