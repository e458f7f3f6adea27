"""Palette-PNG input measurements (rmem_png_decode_labels through rmem_ocu_amd.png); bench.py is not involved.

64 seeded blob annotations (tests/boundary_ref.blobs) written by Pillow (mode P, its default settings) at 480x854 with 10 objects and
at 1080x1920 with 5 objects:
  * device us per frame and files/s: HIP events around `--iters` png.decode_labels_into calls on the 64-file pack after `--warmup`
    calls (the compressed bytes copied from pinned memory inside every call, no synchronisation, labels left on the device);
  * the same including packing (chunk walk, CRC-32s, pinned buffer) and the status readback: a host clock around `--iters`
    png.decode_label_stack calls on the 64 files' bytes;
  * Pillow's np.array(Image.open(file)) on one process and on `--threads` processes (default 16), `--cpu-rounds` passes over the 64
    files, the pool started and warmed before the clock;
  * compressed MB/s, the ratio to the `--threads` Pillow processes, and the share of the 294 us a propagated frame costs at the
    headline rate (3,400 frames/s);
  * whether every decoded frame equals the label map the file was written from.
Prints one JSON line.  Kernel split: run it under `rocprofv3 --kernel-trace --stats -- python scripts/pngdec_bench.py --skip-cpu`.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import boundary_ref as R  # noqa: E402

FRAMES = 64
CASES = (dict(H=480, W=854, objects=10), dict(H=1080, W=1920, objects=5))
FRAME_US_AT_HEADLINE = 294.0


def pillow_write(mask):
    from PIL import Image
    im = Image.fromarray(mask).convert('P')
    im.putpalette(list(range(256)) * 3)
    buf = io.BytesIO()
    im.save(buf, 'PNG')
    return buf.getvalue()


def pillow_read(data):
    """what the reference's dataset does with an annotation file"""
    from PIL import Image
    return int(np.array(Image.open(io.BytesIO(data))).sum())


def pillow_rate(files, rounds, workers):
    work = [files[i % len(files)] for i in range(rounds * len(files))]
    if workers == 1:
        pillow_read(work[0])
        t0 = time.perf_counter()
        for f in work:
            pillow_read(f)
        return len(work) / (time.perf_counter() - t0)
    with ProcessPoolExecutor(workers) as ex:
        list(ex.map(pillow_read, work[:2 * workers]))            # start and warm every worker
        t0 = time.perf_counter()
        list(ex.map(pillow_read, work, chunksize=4))
        return len(work) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cpu-rounds', type=int, default=2)
    ap.add_argument('--skip-cpu', action='store_true')
    args = ap.parse_args()
    res = {'metric': 'png_decode_labels', 'frames': FRAMES, 'cpu_workers': args.threads, 'cases': []}
    stacks, packs, cpu = [], [], []
    for c in CASES:                                           # the host work first: its worker processes never see the device
        stack = np.stack([R.blobs(c['H'], c['W'], c['objects'] + 1, seed=2000 + c['H'] + i) for i in range(FRAMES)])
        files = [pillow_write(m) for m in stack]
        stacks.append(stack)
        packs.append(files)
        if args.skip_cpu:
            cpu.append(None)
            continue
        cpu.append((pillow_rate(files, 1, 1), pillow_rate(files, args.cpu_rounds, args.threads)))
        print(json.dumps(dict(size=f"{c['H']}x{c['W']}", pillow_1=cpu[-1][0], pillow_n=cpu[-1][1])), file=sys.stderr, flush=True)
    import torch
    from rmem_ocu_amd import png
    dev = torch.device('cuda', 0)
    for c, stack, files, cp in zip(CASES, stacks, packs, cpu):
        H, W = c['H'], c['W']
        pk = png.PackedPngs(files)
        out = torch.empty(FRAMES, H, W, dtype=torch.uint8, device=dev)
        for _ in range(args.warmup):
            png.decode_labels_into(pk, out, 0, FRAMES)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            png.decode_labels_into(pk, out, 0, FRAMES)
        b.record()
        torch.cuda.synchronize()
        pk.check(dev)
        sec = a.elapsed_time(b) / 1e3 / args.iters
        ok = bool(torch.equal(out.cpu(), torch.from_numpy(stack)))
        for _ in range(args.warmup):
            png.decode_label_stack(files, dev)
        t0 = time.perf_counter()
        for _ in range(args.iters):
            png.decode_label_stack(files, dev)
        sec_files = (time.perf_counter() - t0) / args.iters
        r = dict(size=f'{H}x{W}', objects=c['objects'], device_us_per_frame=round(1e6 * sec / FRAMES, 2), ms_per_call=round(1e3 * sec, 3),
                 device_files_per_s=round(FRAMES / sec, 1), compressed_bytes_per_frame=round(pk.compressed_bytes / FRAMES, 1),
                 compressed_MB_per_s=round(pk.compressed_bytes / sec / 1e6, 2), label_MB_per_s=round(FRAMES * H * W / sec / 1e6, 1),
                 with_packing_and_readback_files_per_s=round(FRAMES / sec_files, 1),
                 with_packing_and_readback_us_per_frame=round(1e6 * sec_files / FRAMES, 2),
                 share_of_a_propagated_frame=round(1e6 * sec / FRAMES / FRAME_US_AT_HEADLINE, 4), all_frames_equal_the_labels=ok)
        if cp is not None:
            r1, rn = cp
            r.update(pillow_files_per_s_1=round(r1, 1), pillow_files_per_s_n=round(rn, 1), device_over_pillow_n=round(FRAMES / sec / rn, 2),
                     with_packing_over_pillow_n=round(FRAMES / sec_files / rn, 2))
        res['cases'].append(r)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
