#!/usr/bin/env python3
"""rmem_bneck_chain against the two launches it replaces (conv3 + shortcut, then the next conv1) at the geometries of the bench:
layer 1: --images frames of 121 x 213 pixels, 64 -> 256 -> N2 = 64, 128; layer 2: frames of 61 x 107 pixels, 128 -> 512 -> N2 = 128, 256,
and layer 2's first block (the dual form: [b | the 121 x 213 x 256 map at stride 2] -> 512 -> 128).  --reps launches back to back per
event pair, rotating over --sets operand sets (the wide maps are 211 and 107 MB each at 16 images: nothing is found in a cache).
Usage: python scripts/bneck_bench.py [--images 16] [--layers 1 2]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (layer, H, W, K1, Cout, N2, dual: (H2, W2, Cin2, stride2) or None)
CASES = [(1, 121, 213, 64, 256, 64, None), (1, 121, 213, 64, 256, 128, None),
         (2, 61, 107, 128, 512, 128, None), (2, 61, 107, 128, 512, 256, None), (2, 61, 107, 128, 512, 128, (121, 213, 256, 2))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--layers', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--iters', type=int, default=7)
    args = ap.parse_args()
    from rmem_ocu_amd import ops
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    B = args.images
    bf = torch.bfloat16
    r = lambda *s, sc=0.5: (torch.randn(*s, generator=g) * sc).to(bf).to(dev)   # noqa: E731
    for layer, H, W, K1, Cout, N2, dual in CASES:
        if layer not in args.layers:
            continue
        M = B * H * W
        KT = K1 + (dual[2] if dual else 0)
        w3, b3 = r(Cout, KT, sc=0.1), torch.randn(Cout, generator=g).to(dev)
        w1, b1 = r(N2, Cout, sc=0.05), torch.randn(N2, generator=g).to(dev)
        b0 = r(M, K1)
        sc0 = r(B * dual[0] * dual[1], dual[2]) if dual else r(M, Cout)
        unf, fus = [], []
        for _ in range(args.sets):
            b, sc = b0.clone(), sc0.clone()
            y = torch.empty(M, Cout, dtype=bf, device=dev)
            a2 = torch.empty(M, N2, dtype=bf, device=dev)
            if dual:
                kw = dict(H2=dual[0], W2=dual[1], Cin2=dual[2], stride2=dual[3])
                first = ops.conv1x1_dual(b, sc, w3, b3, y, H=H, W=W, Cin=K1, Cout=Cout, relu=True, batch=B, **kw)
                kw['x2'] = sc
            else:
                first = ops.conv2d(b, w3, b3, y, H=H, W=W, Cin=K1, Cout=Cout, residual=sc, relu=True, batch=B)
                kw = dict(residual=sc)
            unf.append([first, ops.conv2d(y, w1, b1, a2, H=H, W=W, Cin=Cout, Cout=N2, relu=True, batch=B)])
            fus.append([ops.bneck_chain(b, w3, b3, y, w1, b1, a2, H=H, W=W, K1=K1, N2=N2, batch=B, Cout=Cout, **kw)])
        for name, sets in (('conv3 + shortcut, conv1 (two launches)', unf), ('rmem_bneck_chain', fus)):
            for s in sets:
                ops.run(s)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(args.reps):
                    ops.run(sets[k % args.sets])
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / args.reps)
            ts.sort()
            # the dual form reads a quarter of its shortcut map's pixels
            mb = (M * (K1 + Cout + N2) + (M * dual[2] if dual else M * Cout)) * 2 / 1e6 + (0 if 'chain' in name else M * Cout * 2 / 1e6)
            t = ts[len(ts) // 2]
            form = 'dual' if dual else 'identity'
            print(f'{B} images, layer {layer} {form}, {K1} -> {Cout} -> {N2}: {name:40s} {t:7.1f} us  ({mb:.0f} MB of compulsory traffic: '
                  f'{mb / t:.2f} TB/s)', flush=True)


if __name__ == '__main__':
    main()
