"""GPU JPEG encode + overlay measurements (rmem_jpeg_encode_rgb8, rmem_ocu_amd/jpeg.py); bench.py is not involved.

Seeded synthetic frames (scripts/jpeg_bench.py's; 16 distinct ones, repeated for the larger batch) with blob labels at 480x854 and
1080x1920, quality 90, in batches of 16 and 64:
  * jpeg.encode_rgb_stack frames/s, without and with labels: wall clock around at least `--iters` calls and `--seconds` seconds
    after `--warmup`, each call ending with the files as bytes on the host (device work + the two device-to-host copies per chunk);
  * the device work alone: HIP events around as many jpeg.encode_files calls;
  * the existing way on `--threads` host threads (default 16): the frames and labels are already host arrays, numpy overlay (with
    labels) + Pillow Image.save per frame; the copy of the frames to the host is NOT in its window;
  * the mean file size, and whether frame 0's entropy-coded segment equals Pillow's byte for byte at this size.
Prints one JSON line.  Share per kernel: run it under `rocprofv3 --kernel-trace --stats -- python scripts/jpegenc_bench.py`.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jpeg_bench import synthetic_frames  # noqa: E402


def blob_labels(n, h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint8)
    for f in range(n):
        for k in range(1, 5):
            cy, cx = rs.uniform(0.2, 0.8) * h, rs.uniform(0.2, 0.8) * w
            ry, rx = rs.uniform(0.1, 0.3) * h, rs.uniform(0.1, 0.3) * w
            out[f][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    return out


def host_overlay(rgb, lab, pal, a=102):
    """the overlay of include/rmem.h in numpy (one frame)"""
    pad = np.pad(lab.astype(np.int16), 1, constant_values=-1)
    m = np.maximum(np.maximum(pad[:-2, 1:-1], pad[2:, 1:-1]), np.maximum(pad[1:-1, :-2], pad[1:-1, 2:]))
    blend = ((a * rgb.astype(np.int32) + (256 - a) * pal[lab] + 128) >> 8).astype(np.uint8)
    out = np.where((lab != 0)[..., None], blend, rgb)
    out[m > lab] = 0
    return out


def pillow_file(a, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', quality=quality, subsampling=2, optimize=False, restart_marker_rows=1)
    return b.getvalue()


def entropy_segment(data):
    at = 2
    while data[at + 1] != 0xDA:
        at += 2 + ((data[at + 2] << 8) | data[at + 3])
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):-2]


def host_rate(frames, labels, pal, quality, threads, seconds):
    """frames/s of numpy overlay (with labels) + Pillow save on `threads` threads: whole passes over `frames` for >= seconds"""
    def one(i):
        return pillow_file(frames[i] if labels is None else host_overlay(frames[i], labels[i], pal), quality)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(len(frames))))                     # warm-up
        t0, reps = time.perf_counter(), 0
        while reps == 0 or time.perf_counter() - t0 < seconds:
            list(ex.map(one, range(len(frames))))
            reps += 1
        dt = time.perf_counter() - t0
    return reps * len(frames) / dt


def device_rates(rgb, lab, quality, warmup, iters, seconds):
    """at least `iters` calls and `seconds` seconds per window"""
    from rmem_ocu_amd import jpeg
    n = rgb.shape[0]
    for _ in range(warmup):
        files = jpeg.encode_rgb_stack(rgb, lab, quality=quality)
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while calls < iters or time.perf_counter() - t0 < seconds:
        files = jpeg.encode_rgb_stack(rgb, lab, quality=quality)    # ends with the files on the host: synchronised
        calls += 1
    dt = time.perf_counter() - t0
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        jpeg.encode_files(rgb, lab, quality=quality)
    b.record()
    torch.cuda.synchronize()
    return files, dict(calls=calls, frames_per_s=round(calls * n / dt, 1),
                       device_only_frames_per_s=round(calls * n / (a.elapsed_time(b) / 1e3), 1),
                       mean_file_kB=round(sum(len(f) for f in files) / n / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5, help='least calls per timed window')
    ap.add_argument('--seconds', type=float, default=0.5, help='least seconds per timed window')
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--skip-host', action='store_true', help='device only (for a kernel trace)')
    args = ap.parse_args()
    from rmem_ocu_amd.evaluator import _davis_palette
    pal = np.array(_davis_palette(), np.int32).reshape(256, 3)
    dev = torch.device('cuda', 0)
    res = {'metric': 'jpeg_encode', 'quality': args.quality, 'host_threads': args.threads, 'cases': []}
    for (h, w) in ((480, 854), (1080, 1920)):
        frames = np.concatenate([np.stack(synthetic_frames(16, h, w, seed=h))] * 4)       # 16 distinct frames, four times
        labels = np.concatenate([blob_labels(16, h, w, seed=h)] * 4)
        print(f'{h}x{w}: inputs ready', file=sys.stderr, flush=True)
        host = None if args.skip_host else {False: host_rate(frames[:16], None, pal, args.quality, args.threads, 2 * args.seconds),
                                            True: host_rate(frames[:16], labels[:16], pal, args.quality, args.threads, 2 * args.seconds)}
        for batch in (16, 64):
            rgb, lab = torch.from_numpy(frames[:batch]).to(dev), torch.from_numpy(labels[:batch]).to(dev)
            for with_labels in (False, True):
                r = dict(size=f'{h}x{w}', batch=batch, overlay=with_labels)
                files, rates = device_rates(rgb, lab if with_labels else None, args.quality, args.warmup, args.iters, args.seconds)
                r.update(rates)
                # at this size too: the device's entropy-coded segment of frame 0 is Pillow's, byte for byte
                want = pillow_file(host_overlay(frames[0], labels[0], pal) if with_labels else frames[0], args.quality)
                r['frame0_equals_pillow'] = entropy_segment(files[0]) == entropy_segment(want)
                if host:
                    r['host_frames_per_s'] = round(host[with_labels], 1)
                    r['speedup_vs_host'] = round(r['frames_per_s'] / host[with_labels], 2)
                res['cases'].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
