"""Shape census measurements (rmem_label_moments, rmem_label_hull_count / _offsets / _write through rmem_ocu_amd.shapes); bench.py
is not involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels, four contents each:
  * blobs       seeded blob annotations with 10 objects (tests/census_ref.blobs);
  * background  all zero: every wave is one run of label 0, no object, no hull;
  * noise       every pixel uniform over 11 ids: every lane's 16 bytes are mixed, every wave holds all 11 and nothing is a run
                (worst divergence); every object is as high as the frame;
  * discs       three discs per frame, the largest of radius 0.48 min(H, W): many hull vertices.
Per stack: us per call, the median of `--iters` calls timed one by one with HIP events on one stream after `--warmup` calls, for
pass A (moments and row extents in one call; each alone too), pass B (hull count, offsets scan and write on pass A's extents,
without the readback of the total) and shapes.region_props end to end (host clock: it ends on the host), and three yardsticks on
the same stack in the same run: rmem_label_census, a device-to-device rmem_copy_async of the same bytes, and the host route the
feature replaces -- stack.cpu(), then numpy moments and the reference hull (tests/shapes_ref.hull) per frame and object.  The host
route is measured on the first `--host-frames` frames and scaled to the stack (frames are independent).  Whether the device tables
equal the host route's on those frames is reported too.  Prints one JSON line.
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
import shapes_ref as R  # noqa: E402

CASES = (dict(n=64, H=480, W=854), dict(n=16, H=1080, W=1920))
CONTENTS = ('blobs', 'background', 'noise', 'discs')
NUM = 10


def make_stack(content, n, H, W):
    if content == 'blobs':
        return census_ref.blobs(1000 + H, n, H, W)
    if content == 'background':
        return np.zeros((n, H, W), dtype=np.uint8)
    if content == 'noise':
        return np.random.default_rng(H).integers(0, 11, (n, H, W)).astype(np.uint8)
    a = np.zeros((n, H, W), dtype=np.uint8)
    r = 0.48 * min(H, W)
    for f in range(n):
        a[f][R.disc(H, W, H / 2 - 0.5, W / 2 - 0.5 + f, r)] = 1
        a[f][R.disc(H, W, H * 0.3, W * 0.25 + f, r * 0.45)] = 2
        a[f][R.disc(H, W, H - 1, W - 1, r * 0.3)] = 3
    return a


def host_route(stack_d, frames):
    """the route the feature replaces, on the first `frames` frames: the stack over PCIe, numpy moments and the hull per object"""
    stack = stack_d[:frames].cpu().numpy()
    verts, off = R.hulls(stack, NUM)
    return R.moments(stack), verts, off


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


def host_us(torch, fn, warmup, iters):
    times = []
    for k in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times[warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-frames', type=int, default=2)
    ap.add_argument('--e2e-iters', type=int, default=5)
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import _lib, ops, shapes
    from rmem_ocu_amd.protocol import label_census
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    res = {'metric': 'label_shapes', 'warmup': args.warmup, 'iters': args.iters, 'num_objs': NUM, 'host_frames': args.host_frames, 'cases': []}
    for c in CASES:
        n, H, W = c['n'], c['H'], c['W']
        nbytes = n * H * W
        for content in CONTENTS:
            stack = torch.from_numpy(make_stack(content, n, H, W)).to(dev)
            out = torch.empty_like(stack)
            s = torch.cuda.current_stream(dev).cuda_stream
            mom = torch.empty(n, 256, 6, dtype=torch.int64, device=dev)
            ext = torch.empty(n, NUM, H, 2, dtype=torch.int32, device=dev)
            flags = torch.empty(n * NUM * (H + 1), dtype=torch.uint8, device=dev)
            off = torch.empty(n * NUM + 1, dtype=torch.int32, device=dev)
            p = stack.data_ptr()

            def pass_b(verts=None):
                _lib.check(L.rmem_label_hull_count(ext.data_ptr(), n, H, W, NUM, flags.data_ptr(), off.data_ptr(), s), 'rmem_label_hull_count')
                _lib.check(L.rmem_label_hull_offsets(off.data_ptr(), n * NUM, s), 'rmem_label_hull_offsets')
                if verts is not None:
                    _lib.check(L.rmem_label_hull_write(ext.data_ptr(), flags.data_ptr(), n, H, W, NUM, off.data_ptr(), verts.data_ptr(),
                                                       verts.shape[0], s), 'rmem_label_hull_write')

            a_us = device_us(torch, lambda: _lib.check(L.rmem_label_moments(p, n, H, W, NUM, mom.data_ptr(), ext.data_ptr(), s), 'A'), args.warmup, args.iters)
            am_us = device_us(torch, lambda: _lib.check(L.rmem_label_moments(p, n, H, W, 0, mom.data_ptr(), None, s), 'A'), args.warmup, args.iters)
            ae_us = device_us(torch, lambda: _lib.check(L.rmem_label_moments(p, n, H, W, NUM, None, ext.data_ptr(), s), 'A'), args.warmup, args.iters)
            pass_b()
            V = int(off[n * NUM].item())
            verts = torch.empty(max(V, 1), 2, dtype=torch.int32, device=dev)
            b_us = device_us(torch, lambda: pass_b(verts if V else None), args.warmup, args.iters)
            count_us = device_us(torch, lambda: _lib.check(L.rmem_label_hull_count(ext.data_ptr(), n, H, W, NUM, flags.data_ptr(), off.data_ptr(), s), 'B'),
                                 args.warmup, args.iters)
            census_us = device_us(torch, lambda: label_census(stack), args.warmup, args.iters)
            copy_us = device_us(torch, lambda: ops.copy_async(out, stack, nbytes)(s), args.warmup, args.iters)
            props_us = host_us(torch, lambda: shapes.region_props(stack, NUM), 1, args.e2e_iters)
            tables_us = host_us(torch, lambda: (shapes.label_moments(stack).cpu(), [t.cpu() for t in shapes.convex_hulls(stack, NUM)]), 1, args.e2e_iters)
            hf = min(args.host_frames, n)
            t0 = time.perf_counter()
            want = host_route(stack, hf)
            host_route_us = (time.perf_counter() - t0) * 1e6 * n / hf
            dv, do = shapes.convex_hulls(stack[:hf], NUM)
            got = (shapes.label_moments(stack[:hf]).cpu().numpy(), dv.cpu().numpy(), do.cpu().numpy())
            equal = all(np.array_equal(g, w) for g, w in zip(got, want))
            res['cases'].append(dict(size=f'{n}x{H}x{W}', content=content, label_MB=round(nbytes / 1e6, 2), hull_vertices=V,
                                     pass_a_us=round(a_us, 1), pass_a_GB_per_s=round(nbytes / a_us / 1e3, 1),
                                     moments_only_us=round(am_us, 1), extents_only_us=round(ae_us, 1),
                                     pass_b_us=round(b_us, 1), hull_count_us=round(count_us, 1),
                                     census_us=round(census_us, 1), copy_us=round(copy_us, 1),
                                     pass_a_over_census=round(a_us / census_us, 2), moments_only_over_census=round(am_us / census_us, 2),
                                     region_props_us=round(props_us, 1), tables_to_host_us=round(tables_us, 1),
                                     host_route_us=round(host_route_us, 1), host_route_over_region_props=round(host_route_us / props_us, 1),
                                     equals_host_route=bool(equal)))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
