#!/usr/bin/env python3
"""ResNet layer 1 as the chained 7-launch list (1x1 conv, 3 x conv3x3_direct, 3 x rmem_bneck_chain) against the 3-launch list of
one-launch bottlenecks (rmem_bneck_block64), at --images frames of 121 x 213 pixels, both element types, timed by HIP events as the
median over --iters pairs of --reps launches of the whole list, rotating over --sets operand sets (a 256-channel map is 211 MB at 16
images: nothing is found in a cache).  Every launch of both lists is also timed alone.  --counters: nothing but a few launches of
the block list at the first --images value in bfloat16, for `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes.
Usage: python scripts/layer1_block_bench.py [--images 16 8] [--counters]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(sets, reps, iters):
    from rmem_ocu_amd import ops
    for s in sets:
        ops.run(s)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(reps):
            ops.run(sets[k % len(sets)])
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, nargs='+', default=[16, 8])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--counters', action='store_true')
    args = ap.parse_args()
    from rmem_ocu_amd import ops
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    H, W = 121, 213
    for dt in (torch.bfloat16,) if args.counters else (torch.bfloat16, torch.float16):
        r = lambda *s, sc=0.5: (torch.randn(*s, generator=g) * sc).to(dt).to(dev)   # noqa: E731
        f = lambda n: (torch.randn(n, generator=g) * 0.1).to(dev)                    # noqa: E731
        blk = []
        for bi in range(3):
            cin = 64 if bi == 0 else 256
            blk.append(dict(w1=r(64, cin, sc=cin ** -0.5), b1=f(64), w2=r(64, 3, 3, 64, sc=1 / 24), b2=f(64),
                            w3=r(256, 128 if bi == 0 else 64, sc=1 / 8), b3=f(256)))
        wn, bn = r(128, 256, sc=1 / 16), f(128)
        for B in args.images[:1] if args.counters else args.images:
            M = B * H * W
            e = lambda c: torch.empty(M, c, dtype=dt, device=dev)                   # noqa: E731
            pool0 = r(M, 64)
            old, new = [], []
            for _ in range(args.sets):
                pool, a, b, xa, xb, a2 = pool0.clone(), e(128), e(64), e(256), e(256), e(128)
                k0, k1, k2 = blk
                g3 = dict(H=H, W=W, C=64, images=B, relu=True)
                old.append([
                    ops.conv2d(pool, k0['w1'], k0['b1'], a, H=H, W=W, Cin=64, Cout=64, relu=True, batch=B),
                    ops.conv3x3_direct(a, k0['w2'], k0['b2'], b, **g3),
                    ops.bneck_chain(b, k0['w3'], k0['b3'], xa, k1['w1'], k1['b1'], a, H=H, W=W, K1=64, N2=64, x2=pool, H2=H, W2=W, Cin2=64,
                                    stride2=1, batch=B),
                    ops.conv3x3_direct(a, k1['w2'], k1['b2'], b, **g3),
                    ops.bneck_chain(b, k1['w3'], k1['b3'], xb, k2['w1'], k2['b1'], a, H=H, W=W, K1=64, N2=64, residual=xa, batch=B),
                    ops.conv3x3_direct(a, k2['w2'], k2['b2'], b, **g3),
                    ops.bneck_chain(b, k2['w3'], k2['b3'], xa, wn, bn, a, H=H, W=W, K1=64, N2=128, residual=xb, batch=B)])
                xc = e(256)
                bb = lambda k, x, y, cin, **kw: ops.bneck_block64(x, k['w1'], k['b1'], k['w2'], k['b2'], k['w3'], k['b3'], y,   # noqa: E731
                                                                  H=H, W=W, Cin=cin, images=B, **kw)
                new.append([bb(k0, pool, xc, 64), bb(k1, xc, xb, 256), bb(k2, xb, xc, 256, w1n=wn, bias1n=bn, a_next=a2)])
            if args.counters:
                for k in range(5):
                    ops.run(new[k % len(new)])
                torch.cuda.synchronize()
                continue
            t_old, t_new = timed(old, args.reps, args.iters), timed(new, args.reps, args.iters)
            tag = f'{str(dt)[6:]:8s} {B:2d} images'
            print(f'{tag}: 7-launch chained list {t_old:7.1f} us   3-launch block list {t_new:7.1f} us   ({t_old / t_new:.2f} x)', flush=True)
            for name, sets in (('old', old), ('new', new)):
                for i in range(len(sets[0])):
                    t = timed([[s[i]] for s in sets], args.reps, args.iters)
                    print(f'{tag}:   {name} launch {i} {sets[0][i].name:24s} {t:7.1f} us', flush=True)


if __name__ == '__main__':
    main()
