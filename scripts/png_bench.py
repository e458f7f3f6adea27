"""Palette-PNG output measurements (rmem_png_encode_labels through rmem_ocu_amd.png); bench.py is not involved.

64 seeded frames of blob label maps (tests/boundary_ref.blobs) at 480x854 with 10 objects and at 1080x1920 with 5 objects:
  * device frames/s and us per frame: HIP events around `--iters` png.encode_zlib calls on the 64-frame stack after `--warmup`
    calls (labels already on the device, streams left on the device);
  * the same with the two readbacks and the host `wrap` included: a host clock around `--iters` png.encode_label_stack calls
    (each ends in a stream synchronise and returns the 64 files);
  * Pillow's save_mask-equivalent (fromarray, convert('P'), putpalette, save as PNG into memory) on one process and on
    `--threads` processes (default 16), `--cpu-rounds` passes over the 64 frames, the pool started and warmed before the clock;
  * mean file bytes against Pillow's and against the raw H * W bytes;
  * whether every device-encoded file decoded (Pillow) back to its label map.
Prints one JSON line.  Kernel split: run it under `rocprofv3 --kernel-trace --stats -- python scripts/png_bench.py --skip-cpu`.
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
_PALETTE = None


def pillow_png(mask):
    """what evaluator.save_mask does, into memory"""
    global _PALETTE
    from PIL import Image
    if _PALETTE is None:
        from rmem_ocu_amd.evaluator import _davis_palette
        _PALETTE = _davis_palette()
    im = Image.fromarray(mask).convert('P')
    im.putpalette(_PALETTE)
    buf = io.BytesIO()
    im.save(buf, 'PNG')
    return buf.getbuffer().nbytes


def pillow_rate(stack, rounds, workers):
    work = [stack[i % len(stack)] for i in range(rounds * len(stack))]
    if workers == 1:
        pillow_png(work[0])
        t0 = time.perf_counter()
        sizes = [pillow_png(m) for m in work]
        return len(work) / (time.perf_counter() - t0), sizes
    with ProcessPoolExecutor(workers) as ex:
        list(ex.map(pillow_png, work[:2 * workers]))             # start and warm every worker
        t0 = time.perf_counter()
        sizes = list(ex.map(pillow_png, work, chunksize=4))
        return len(work) / (time.perf_counter() - t0), sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cpu-rounds', type=int, default=2)
    ap.add_argument('--skip-cpu', action='store_true')
    args = ap.parse_args()
    res = {'metric': 'png_encode_labels', 'frames': FRAMES, 'cpu_workers': args.threads, 'cases': []}
    stacks, cpu = [], []
    for c in CASES:                                           # the host work first: its worker processes never see the device
        stack = np.stack([R.blobs(c['H'], c['W'], c['objects'] + 1, seed=2000 + c['H'] + i) for i in range(FRAMES)])
        stacks.append(stack)
        if args.skip_cpu:
            cpu.append(None)
            continue
        r1, sizes = pillow_rate(stack, 1, 1)
        rn, _ = pillow_rate(stack, args.cpu_rounds, args.threads)
        cpu.append((r1, rn, float(np.mean(sizes))))
        print(json.dumps(dict(size=f"{c['H']}x{c['W']}", pillow_1=r1, pillow_n=rn)), file=sys.stderr, flush=True)
    import torch
    from PIL import Image
    from rmem_ocu_amd import png
    dev = torch.device('cuda', 0)
    for c, stack, cp in zip(CASES, stacks, cpu):
        H, W = c['H'], c['W']
        lab = torch.from_numpy(stack).to(dev)
        for _ in range(args.warmup):
            out, offsets = png.encode_zlib(lab)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            out, offsets = png.encode_zlib(lab)
        b.record()
        torch.cuda.synchronize()
        sec = a.elapsed_time(b) / 1e3 / args.iters
        for _ in range(args.warmup):
            files = png.encode_label_stack(lab)
        t0 = time.perf_counter()
        for _ in range(args.iters):
            files = png.encode_label_stack(lab)
        sec_files = (time.perf_counter() - t0) / args.iters
        ok = all(np.array_equal(np.array(Image.open(io.BytesIO(f))), stack[i]) for i, f in enumerate(files))
        stream_bytes = int(offsets[-1].item())
        bound = FRAMES * (2 + (3 + 9 * (W + 1) * H + 7 + 7) // 8 + 4)
        file_bytes = float(np.mean([len(f) for f in files]))
        r = dict(size=f'{H}x{W}', objects=c['objects'], device_frames_per_s=round(FRAMES / sec, 1),
                 device_us_per_frame=round(1e6 * sec / FRAMES, 2), ms_per_call=round(1e3 * sec, 3),
                 files_frames_per_s=round(FRAMES / sec_files, 1), files_us_per_frame=round(1e6 * sec_files / FRAMES, 2),
                 file_bytes_mean=round(file_bytes, 1), raw_bytes=H * W, file_over_raw=round(file_bytes / (H * W), 4),
                 stream_bytes_per_frame=round(stream_bytes / FRAMES, 1), stream_over_bound=round(stream_bytes / bound, 4),
                 label_bytes_read_per_frame=2 * 2 * H * W, floor_us_per_frame_at_6p3_TBps=round(2 * 2 * H * W / 6.3e6, 3),
                 all_files_decode_to_labels=bool(ok))
        if cp is not None:
            r1, rn, pil_bytes = cp
            r.update(pillow_frames_per_s_1=round(r1, 1), pillow_frames_per_s_n=round(rn, 1), pillow_file_bytes_mean=round(pil_bytes, 1),
                     file_over_pillow=round(file_bytes / pil_bytes, 3), device_speedup_vs_pillow_n=round(FRAMES / sec / rn, 1),
                     files_speedup_vs_pillow_n=round(FRAMES / sec_files / rn, 2))
        res['cases'].append(r)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
