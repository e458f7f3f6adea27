"""Pair census measurements (rmem_label_pair_census through rmem_ocu_amd.pairs.pair_census); bench.py is not involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels, three contents each (a against b):
  * blobs       seeded blob annotations with 10 objects (tests/census_ref.blobs) against the same blobs moved by (2, 3) pixels: what
                a prediction against its annotation looks like;
  * background  all zero against all zero: every wave of every workgroup meets on one bin (worst contention);
  * noise       every pixel uniform over 11 ids in both: every lane's 16 pixels are mixed and every wave holds all 121 pairs (worst
                divergence).
and num_a = num_b of 10 (table in LDS) and of 255 (table in global memory).  Per case: us per call and GB/s of label bytes (both
stacks), the median of `--iters` calls timed one by one with HIP events on one stream after `--warmup` calls, and three yardsticks
on the same stacks in the same run, because no earlier commit has this route:
  (a) copy    a device-to-device rmem_copy_async of both stacks;
  (b) torch   the torch route on the device: per frame torch.bincount(a.long() * (num_b + 2) + b.long()) after the clamps;
  (c) host    .cpu() of both stacks plus numpy bincount, on the first 2 frames (median of `--cpu-rounds` passes on a host clock;
              reported per 2 frames and scaled to the stack by n / 2).
Whether the three routes give the same table is reported too.  Prints one JSON line.
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

import census_ref as R  # noqa: E402

CASES = (dict(n=64, H=480, W=854), dict(n=16, H=1080, W=1920))
CONTENTS = ('blobs', 'background', 'noise')
NUMS = (10, 255)
HOST_FRAMES = 2


def make_stacks(content, n, H, W):
    if content == 'blobs':
        a = R.blobs(1000 + H, n, H, W)
        return a, np.roll(a, (2, 3), axis=(1, 2))
    if content == 'background':
        return np.zeros((n, H, W), dtype=np.uint8), np.zeros((n, H, W), dtype=np.uint8)
    rng = np.random.default_rng(H)
    return rng.integers(0, 11, (n, H, W)).astype(np.uint8), rng.integers(0, 11, (n, H, W)).astype(np.uint8)


def torch_route(torch, a, b, num_a, num_b):
    """the table with torch alone, on the device: clamp, widen, one bincount per frame"""
    bins = (num_a + 2) * (num_b + 2)
    out = []
    for f in range(a.shape[0]):
        key = a[f].long().clamp_(max=num_a + 1) * (num_b + 2) + b[f].long().clamp_(max=num_b + 1)   # num + 1 = 256 is no uint8
        out.append(torch.bincount(key.reshape(-1), minlength=bins))
    return torch.stack(out).view(a.shape[0], num_a + 2, num_b + 2)


def host_route(a_d, b_d, num_a, num_b):
    """what the device table replaces: both stacks over PCIe, numpy bincount per frame"""
    a, b = a_d.cpu().numpy(), b_d.cpu().numpy()
    bins = (num_a + 2) * (num_b + 2)
    out = np.empty((a.shape[0], num_a + 2, num_b + 2), dtype=np.int64)
    for f in range(a.shape[0]):
        key = np.minimum(a[f].astype(np.int64), num_a + 1) * (num_b + 2) + np.minimum(b[f].astype(np.int64), num_b + 1)
        out[f] = np.bincount(key.reshape(-1), minlength=bins).reshape(num_a + 2, num_b + 2)
    return out


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
    ap.add_argument('--cpu-rounds', type=int, default=3)
    ap.add_argument('--cases', type=int, default=len(CASES), help='the first CASES only (a rehearsal)')
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import _lib, ops
    from rmem_ocu_amd.pairs import pair_census
    if not torch.cuda.is_available():
        raise SystemExit('pair_census_bench: no GPU')
    dev = torch.device('cuda', 0)
    res = {'metric': 'label_pair_census', 'warmup': args.warmup, 'iters': args.iters,
           'lds_bins': int(_lib.lib().rmem_label_pair_census_lds_bins()), 'host_frames': HOST_FRAMES, 'cases': []}
    for c in CASES[:args.cases]:
        n, H, W = c['n'], c['H'], c['W']
        nbytes = 2 * n * H * W
        for content in CONTENTS:
            a, b = (torch.from_numpy(t).to(dev) for t in make_stacks(content, n, H, W))
            ca, cb = torch.empty_like(a), torch.empty_like(b)
            stream = torch.cuda.current_stream(dev).cuda_stream

            def copy():
                ops.copy_async(ca, a, a.numel())(stream)
                ops.copy_async(cb, b, b.numel())(stream)

            copy_us = device_us(torch, copy, args.warmup, args.iters)
            for num in NUMS:
                pairs_us = device_us(torch, lambda: pair_census(a, b, num, num), args.warmup, args.iters)
                torch_us = device_us(torch, lambda: torch_route(torch, a, b, num, num), args.warmup, args.iters)
                host, want = [], None
                for _ in range(args.cpu_rounds):
                    t0 = time.perf_counter()
                    want = host_route(a[:HOST_FRAMES], b[:HOST_FRAMES], num, num)
                    host.append((time.perf_counter() - t0) * 1e6)
                got = pair_census(a, b, num, num).cpu().numpy()
                equal = bool(np.array_equal(got, torch_route(torch, a, b, num, num).cpu().numpy())
                             and np.array_equal(got[:HOST_FRAMES], want))
                host_us = float(np.median(host)) * n / HOST_FRAMES

                def gbs(us):
                    return round(nbytes / us / 1e3, 1)

                res['cases'].append(dict(size=f'{n}x{H}x{W}', content=content, num=num,
                                         route='lds' if (num + 2) ** 2 <= res['lds_bins'] else 'global',
                                         label_MB=round(nbytes / 1e6, 2), pairs_us=round(pairs_us, 1), pairs_GB_per_s=gbs(pairs_us),
                                         copy_us=round(copy_us, 1), copy_GB_per_s=gbs(copy_us), torch_us=round(torch_us, 1),
                                         host_us_scaled=round(host_us, 1), pairs_over_copy=round(pairs_us / copy_us, 2),
                                         torch_over_pairs=round(torch_us / pairs_us, 1), host_over_pairs=round(host_us / pairs_us, 1),
                                         equals_torch_and_host_routes=equal))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
