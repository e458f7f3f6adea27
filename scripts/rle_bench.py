"""COCO run-length mask measurements (rmem_rle_encode_labels / rmem_rle_decode_labels through rmem_ocu_amd.rle); bench.py is not
involved.

Stacks of 64 x 480 x 854 and 16 x 1080 x 1920 uint8 labels, the three contents of census_bench.py: blobs (10 objects), background
(all zero), noise (every pixel uniform over 11 ids: a run boundary at nearly every pixel, the worst case of the format), num_ids 10.
Per stack, for both directions:
  * device calls: us per pass over the stack and GB/s of label bytes, the median of `--iters` passes timed one by one with HIP events
    on one stream after `--warmup` passes.  A pass is what encode_label_stack / decode_label_stack enqueue (encode in chunks of
    rle.frames_per_call frames, with a capacity that fits; decode with its copy of the strings from pinned memory), without the
    readback and the host's dict building;
  * end to end on a host clock, the median of `--e2e-rounds`: rle.encode_label_stack from the device stack to the per-frame dicts
    (with its retry when the default capacity is too small), rle.decode_label_stack from the dicts to the device stack;
  * yardsticks on the same stack in the same run: a device-to-device rmem_copy_async of the label bytes, and the host route the
    device route replaces, on the first `--cpu-frames` frames only (it is slow) and reported per frame: stack.cpu(), then per
    object a numpy run-length pass and numpy string building; for decode numpy parsing and painting per object, then the upload;
  * bytes that cross PCIe on both routes, and whether the device's strings equal the host route's (on the frames it ran).
Prints one JSON line.
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
K = 10


def make_stack(content, n, H, W):
    if content == 'blobs':
        return R.blobs(1000 + H, n, H, W)
    if content == 'background':
        return np.zeros((n, H, W), dtype=np.uint8)
    return np.random.default_rng(H).integers(0, 11, (n, H, W)).astype(np.uint8)


def host_string(mask):
    """numpy throughout: the counts of a binary mask [H, W] read column-major, then maskApi.c's string"""
    flat = mask.T.reshape(-1)
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate(([0], edges, [flat.size]))).astype(np.int64)
    if flat[0]:
        counts = np.concatenate(([0], counts))
    x = counts.copy()
    x[3:] -= counts[1:-2]
    chars = np.zeros((x.size, 6), dtype=np.uint8)
    alive = np.ones(x.size, dtype=bool)
    valid = np.zeros((x.size, 6), dtype=bool)
    for k in range(6):
        c = x & 0x1f
        x = x >> 5
        more = np.where(c & 0x10, x != -1, x != 0)
        chars[:, k] = c + 48 + 32 * more
        valid[:, k] = alive
        alive = alive & more
    return chars[valid].tobytes()


def host_encode(stack_d, frames):
    stack = stack_d[:frames].cpu().numpy()
    return [[host_string(fr == k) for k in range(1, K + 1)] for fr in stack]


def host_mask(string, H, W):
    """numpy throughout: the binary mask of a string"""
    c = np.frombuffer(string, dtype=np.uint8).astype(np.int64) - 48
    ends = (c & 0x20) == 0
    starts = np.concatenate(([0], np.flatnonzero(ends)[:-1] + 1))
    k = np.arange(c.size) - np.repeat(starts, np.diff(np.concatenate((starts, [c.size]))))
    x = np.add.reduceat((c & 0x1f) << (5 * k), starts)
    last = np.flatnonzero(ends)
    x = np.where(c[last] & 0x10, x | (-1 << (5 * (k[last] + 1))), x)
    counts = x.copy()
    counts[3::2] = np.cumsum(x[1::2])[1:]
    counts[2::2] = np.cumsum(x[2::2])
    value = (np.arange(counts.size) & 1).astype(np.uint8)
    return np.repeat(value, counts).reshape(W, H).T


def host_decode(frames, H, W, dev, torch):
    out = np.zeros((len(frames), H, W), dtype=np.uint8)
    for f, fr in enumerate(frames):
        for k, r in fr.items():
            out[f][host_mask(r['counts'], H, W) != 0] = k
    return torch.from_numpy(out).to(dev)


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


def host_us(torch, fn, rounds):
    times, res = [], None
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--e2e-rounds', type=int, default=3)
    ap.add_argument('--cpu-frames', type=int, default=2)
    ap.add_argument('--cpu-rounds', type=int, default=2)
    args = ap.parse_args()
    import torch
    from rmem_ocu_amd import ops, rle
    dev = torch.device('cuda', 0)
    res = {'metric': 'rle', 'num_ids': K, 'warmup': args.warmup, 'iters': args.iters, 'e2e_rounds': args.e2e_rounds,
           'cpu_frames': args.cpu_frames, 'workspace_cap_MB': rle.WORKSPACE_CAP >> 20, 'cases': []}
    for c in CASES:
        n, H, W = c['n'], c['H'], c['W']
        nbytes = n * H * W
        step = rle.frames_per_call(H, W, K)
        for content in CONTENTS:
            stack = torch.from_numpy(make_stack(content, n, H, W)).to(dev)
            scratch = torch.empty_like(stack)
            stream = torch.cuda.current_stream(dev).cuda_stream
            frames = rle.encode_label_stack(stack, K)                     # the strings, through the whole device route
            string_bytes = sum(len(r['counts']) for fr in frames for r in fr.values())
            caps = [sum(len(r['counts']) for fr in frames[k:k + step] for r in fr.values()) for k in range(0, n, step)]

            def encode_pass():
                for i, k in enumerate(range(0, n, step)):
                    rle.encode(stack[k:k + step], K, caps[i])

            packed = rle.PackedRles(frames, (H, W))
            back = torch.empty_like(stack)
            encode_us = device_us(torch, encode_pass, args.warmup, args.iters)
            decode_us = device_us(torch, lambda: rle.decode_labels_into(packed, back), args.warmup, args.iters)
            packed.check(dev)
            round_trip = bool(torch.equal(back, stack))
            copy_us = device_us(torch, lambda: ops.copy_async(scratch, stack, nbytes)(stream), args.warmup, args.iters)
            encode_e2e_us, _ = host_us(torch, lambda: rle.encode_label_stack(stack, K), args.e2e_rounds)
            decode_e2e_us, _ = host_us(torch, lambda: rle.decode_label_stack(frames, (H, W), dev), args.e2e_rounds)
            m = min(n, args.cpu_frames)
            host_enc_us, host_strings = host_us(torch, lambda: host_encode(stack, m), args.cpu_rounds)
            host_dec_us, host_back = host_us(torch, lambda: host_decode(frames[:m], H, W, dev, torch), args.cpu_rounds)
            equal = host_strings == [[fr[k]['counts'] for k in range(1, K + 1)] for fr in frames[:m]]
            host_decode_equal = bool(torch.equal(host_back, stack[:m]))

            def gbs(us):
                return round(nbytes / us / 1e3, 2)

            res['cases'].append(dict(
                size=f'{n}x{H}x{W}', content=content, label_MB=round(nbytes / 1e6, 2), frames_per_call=step, string_bytes=string_bytes,
                encode_us=round(encode_us, 1), encode_GB_per_s=gbs(encode_us), decode_us=round(decode_us, 1), decode_GB_per_s=gbs(decode_us),
                copy_us=round(copy_us, 1), copy_GB_per_s=gbs(copy_us),
                encode_over_copy=round(encode_us / copy_us, 1), decode_over_copy=round(decode_us / copy_us, 1),
                encode_end_to_end_us_per_frame=round(encode_e2e_us / n, 1), decode_end_to_end_us_per_frame=round(decode_e2e_us / n, 1),
                host_encode_us_per_frame=round(host_enc_us / m, 1), host_decode_us_per_frame=round(host_dec_us / m, 1),
                host_over_device_encode=round((host_enc_us / m) / (encode_e2e_us / n), 1),
                host_over_device_decode=round((host_dec_us / m) / (decode_e2e_us / n), 1),
                pcie_bytes_device_encode=string_bytes + 8 * (n * K + -(-n // step)), pcie_bytes_host_encode=nbytes,
                pcie_bytes_device_decode=string_bytes + 28 * n * K, pcie_bytes_host_decode=nbytes,
                strings_equal_host_route=bool(equal), host_decode_equals_stack=host_decode_equal, device_round_trip_equal=round_trip))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
