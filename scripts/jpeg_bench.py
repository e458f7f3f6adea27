"""GPU JPEG decode measurements (rmem_jpeg_decode_batch, rmem_ocu_amd/jpeg.py); bench.py is not involved.

Seeded synthetic frames encoded by Pillow (4:2:0) at 480x854 and 1080x1920, quality 90 and 95, in batches of 16 and 64:
  * device decode images/s and compressed MB/s: HIP events around `--iters` decode calls after `--warmup` (the compressed bytes
    are already on the device; the H2D copy is not in the window);
  * rmem_jpeg_pack cost per frame on the host (once per clip load, not on the timed path);
  * Pillow decode images/s on `--threads` host threads (default 16), in the same call;
  * sync statistics per decode call: cross-workgroup sync launches that ran, units sent to the sequential fallback.
Then the end-to-end frames/s of a GroupSlot workload (B clips, R50-AOTL, encoder look-ahead 2) fed by JpegClips next to the same
workload fed by Pillow-decoded pinned uint8 frames.  Prints one JSON line.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python scripts/jpeg_bench.py`.
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


def synthetic_frames(n, h, w, seed):
    """smooth colour fields with edges and mild noise (compresses like camera frames, not like noise)"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        low = torch.rand(1, 3, 9, 16, generator=g) * 255
        img = F.interpolate(low, size=(h, w), mode='bicubic', align_corners=False)[0]
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        for _ in range(6):                                  # a few hard-edged discs
            cy, cx, r = (torch.rand(3, generator=g) * torch.tensor([h, w, h / 4])).tolist()
            img[:, (yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = (torch.rand(3, 1, generator=g) * 255)
        img = img + torch.randn(3, h, w, generator=g) * 4
        out.append(img.clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy())
    return out


def encode(a, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', quality=quality, subsampling=2)
    return b.getvalue()


def pillow_rate(datas, threads, reps):
    from PIL import Image

    def dec(d):
        return np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(dec, datas))                          # warm-up
        t0 = time.perf_counter()
        for _ in range(reps):
            list(ex.map(dec, datas))
        dt = time.perf_counter() - t0
    return reps * len(datas) / dt


def device_decode(datas, dev, warmup, iters):
    from rmem_ocu_amd import jpeg
    p = jpeg.PackedJpegs(datas)
    h, w = p.sizes[0]
    out = torch.empty(len(datas), h, w, 3, dtype=torch.uint8, device=dev)
    outs = list(out)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    p.decode_into(outs, 0, len(datas))
    p.check(dev)
    for _ in range(warmup):
        p.decode_into(outs, 0, len(datas), upload=False)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        p.decode_into(outs, 0, len(datas), upload=False, stats=stats)
    b.record()
    torch.cuda.synchronize()
    p.check(dev)
    sec = a.elapsed_time(b) / 1e3
    st = stats.cpu().tolist()
    return dict(images_per_s=round(iters * len(datas) / sec, 1), compressed_MB_per_s=round(iters * p.compressed_bytes / sec / 1e6, 1),
                ms_per_call=round(1e3 * sec / iters, 3), pack_us_per_frame=round(1e6 * p.pack_seconds / len(datas), 1),
                mean_compressed_kB=round(p.compressed_bytes / len(datas) / 1e3, 1),
                sync_launches_per_call=round(st[0] / iters, 2), fallback_units_per_call=round(st[1] / iters, 3))


def group_slot_fps(srcs, masks, model, dev, B, reps):
    from rmem_ocu_amd.clip_runner import GroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    ge = GroupEngine(model, B, 0, 5, lookahead=2)
    gs = GroupSlot(ge, tuple(srcs[0].shape[1:3]), dev)
    best = 0.0
    for r in range(reps + 1):                             # run 0 warms up (graphs, workspaces)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gs.start(srcs, masks, 2)
        while not gs.done:
            gs.step()
        ge.synchronize()
        dt = time.perf_counter() - t0
        if r:
            best = max(best, B * (int(srcs[0].shape[0]) - 1) / dt)
    return round(best, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--e2e-clips', type=int, default=4)
    ap.add_argument('--e2e-frames', type=int, default=33)
    ap.add_argument('--skip-e2e', action='store_true')
    args = ap.parse_args()
    from rmem_ocu_amd.jpeg import JpegClip
    dev = torch.device('cuda', 0)
    res = {'metric': 'jpeg_decode', 'pillow_threads': args.threads, 'cases': []}
    for (h, w) in ((480, 854), (1080, 1920)):
        imgs = synthetic_frames(64, h, w, seed=h)
        for q in (90, 95):
            datas = [encode(a, q) for a in imgs]
            pil = pillow_rate(datas[:16], args.threads, 3)
            for batch in (16, 64):
                r = dict(size=f'{h}x{w}', quality=q, batch=batch)
                r.update(device_decode(datas[:batch], dev, args.warmup, args.iters))
                r['pillow_images_per_s'] = round(pil, 1)
                r['speedup_vs_pillow'] = round(r['images_per_s'] / pil, 2)
                res['cases'].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    if not args.skip_e2e:
        import torch.nn.functional as F
        from PIL import Image
        from rmem_ocu_amd import build_vos_model, get_config
        from rmem_ocu_amd.synth import make_clip, network_size
        from rmem_ocu_amd.weights import synth_state_dict
        cfg = get_config('pre_vost', 'test', 'r50_aotl')
        model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
        model.load_state_dict(synth_state_dict(0))
        video = (480, 854)
        net = network_size(*video)
        u8s, jpgs, masks = [], [], []
        for c in range(args.e2e_clips):
            f, m = make_clip(500 + c, args.e2e_frames, net[0], net[1], 2)
            v = F.interpolate(f, size=video, mode='bilinear', align_corners=False)
            u8 = (v * 40.0 + 128.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
            datas = [encode(u8[k], 90) for k in range(len(u8))]
            dec = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas])
            u8s.append(torch.from_numpy(dec).pin_memory())
            jpgs.append(JpegClip(datas))
            masks.append(m.to(dev))
        e2e = {'clips': args.e2e_clips, 'frames_per_clip': args.e2e_frames, 'video_hw': list(video), 'network_hw': list(net)}
        e2e['pinned_uint8_fps'] = group_slot_fps(u8s, masks, model, dev, args.e2e_clips, 2)
        e2e['jpeg_clip_fps'] = group_slot_fps(jpgs, masks, model, dev, args.e2e_clips, 2)
        for j in jpgs:
            j.check(dev)
        e2e['compressed_vs_rgb_bytes'] = round(sum(j.compressed_bytes for j in jpgs) / sum(u.numel() for u in u8s), 4)
        res['group_slot_e2e'] = e2e
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
