"""The frozen image encoders over several frames at once (ResNet-50: BatchEncoder, Swin-B: SwinBatchEncoder).

Clips are independent but share the frozen encoder (encoders/resnet.py:10-196; models/aot.py:116-134), and one 481x849
frame gives GEMMs of only 1.7 k - 26 k rows.  ``BatchEncoder`` runs every encoder layer once for B frames (the conv
kernel's ``batch`` dimension: rows are [image][ho][wo]), writing the three stage outputs into [B, ...] buffers ``enc_out``
(enc1, enc2, enc3) that the runtime's launch lists -- projector, LSTT, decoder -- continue from (GroupRuntime._enc).  A frame's
results do not depend on B: the same kernel computes every output row from the same operands in the same order.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

from . import ops
from .pack import R50_BLOCKS, R50_STRIDES
from .runtime import BF16, F32, _out


class _PtrInput:
    """Input side of the batch encoders: the frames are named by a device table of pointers (one fp32 [3, H, W] frame each,
    wherever the caller keeps its clips) that set_frames() re-sends before a launch; img_in remains as a staging buffer for
    callers that copy their frames in (point_at_img_in: the default state)."""

    def _init_ptrs(self, B: int, device):
        self.img_ptrs = torch.tensor([self.img_in[i].data_ptr() for i in range(B)], dtype=torch.int64).to(device)
        self._ptr_ring = ops.PinnedRing(4, (B,), torch.int64, device)
        self._ptrs_set = False              # True: the table names caller-owned frames (set_frames), not img_in

    def _input_op(self):
        return ops.image_ptrs_to_nhwc8(self.img_ptrs, self.img8, H=self.H, W=self.W, images=self.B)

    def set_frames(self, frames, stream: int):
        """frames: B fp32 [3, H, W] contiguous device tensors (kept alive by the caller until the encoder launch has run)."""
        assert len(frames) == self.B
        host = self._ptr_ring.next()
        for i, f in enumerate(frames):
            assert f.dtype == F32 and f.is_contiguous() and f.numel() == 3 * self.H * self.W
            host[i] = f.data_ptr()
        self._ptr_ring.upload(self.img_ptrs, self.B * 8, stream)
        self._ptrs_set = True

    def point_at_img_in(self, stream: int):
        """the table names the rows of img_in again (callers that fill img_in themselves)"""
        if self._ptrs_set:
            self.set_frames([self.img_in[i] for i in range(self.B)], stream)
            self._ptrs_set = False


@dataclass(frozen=True)
class EncoderRoutes:
    """Which launches BatchEncoder builds its list from.  Every route computes the same maps, bit for bit, except stem='rowrun'
    (another summation order) and front_split > 1 (split-K plans follow the GEMM's row count)."""
    # 'pool': stem + max-pool in one pass (the half-resolution map is never written) | 'direct': stem and max-pool as two launches |
    # 'rowrun': the 8-channel input layout and the generic row-run GEMM form (experiments; the only form of a pack without stem.w4)
    stem: str = 'pool'
    # n (experiment): stem and layer 1 run depth-first over n sub-batches of B / n frames (their maps are 211 MB per 16 frames: a
    # sub-batch's maps may stay in the Infinity Cache between producer and consumer), layers 2-3 over all B frames; 1 unless n divides B
    front_split: int = 1
    # layer 1: every bottleneck is ONE launch (rmem_bneck_block64: the block's input read once, its output written once, the 64-channel
    # maps never leave the CU), the last one with layer 2's first conv1 as its tail; off: the chained list.  Needs layer 1 in `chain`
    block1: bool = True
    # layers 1 and 2 (256-channel maps at stride 4, 512-channel maps at stride 8, 107 MB each at 16 frames: HBM-bound at these batch
    # sizes): a block's conv3 + shortcut is chained into the NEXT block's conv1 in one launch (rmem_bneck_chain): the wide map is
    # written once, not read back by that conv1.  A layer that is not listed takes separate launches
    chain: Tuple[int, ...] = (1, 2)
    # planes whose stride-1 3x3 is rmem_conv3x3_direct: layer 1 (64 channels); the 128-channel form (layer 2) is faster alone
    # (57.3 -> 43.5 us) but takes a whole CU's LDS per workgroup and measured neutral in the pipeline: opt-in
    direct3: Tuple[int, ...] = (64,)

    @classmethod
    def from_env(cls, env=os.environ) -> 'EncoderRoutes':
        """The RMEM_* switches of the batch encoder; the on / off ones act at the value '1' only."""
        on = lambda k: env.get(k, '0') == '1'       # noqa: E731
        stem = env.get('RMEM_STEM', 'pool')
        chain = () if on('RMEM_NO_BNECK_CHAIN') else (1,) if on('RMEM_NO_BNECK_CHAIN2') else (1, 2)
        return cls(stem=stem if stem in ('pool', 'rowrun') else 'direct', front_split=int(env.get('RMEM_ENC_FRONT_SPLIT', '1')),
                   block1=bool(chain) and not on('RMEM_NO_BNECK_BLOCK'), chain=chain,
                   direct3=() if on('RMEM_NO_DIRECT_CONV3') else (64, 128) if on('RMEM_DIRECT_CONV3_128') else (64,))


def r50_steps(routes: EncoderRoutes, blocks=R50_BLOCKS) -> list:
    """The launches of the bottleneck stack in order, i counting the blocks through the layers: ('block', i, tail) the whole block
    (tail: with block i + 1's conv1), ('conv1', i), ('conv2', i, direct), ('chain', i) conv3 + shortcut with block i + 1's conv1,
    ('conv3', i) conv3 + shortcut alone.  Block i's conv1 is a step of its own unless the step before it was a chain or a tail."""
    layer = [li for li, n in enumerate(blocks, start=1) for _ in range(n)]
    steps, fed = [], False
    for i, li in enumerate(layer):
        last = i + 1 == len(layer)
        if routes.block1 and li == 1:
            fed = not last and layer[i + 1] != li
            steps.append(('block', i, fed))
            continue
        if not fed:
            steps.append(('conv1', i))
        stride = R50_STRIDES[li - 1] if i == 0 or layer[i - 1] != li else 1
        steps.append(('conv2', i, 64 * 2 ** (li - 1) in routes.direct3 and stride == 1))
        fed = li in routes.chain and not last
        steps.append(('chain' if fed else 'conv3', i))
    return steps


class BatchEncoder(_PtrInput):
    def __init__(self, P: Dict[str, torch.Tensor], in_hw: Tuple[int, int], batch: int, device, routes: Optional[EncoderRoutes] = None):
        if 'pe.w' in P:
            raise ops.RmemError('BatchEncoder covers the ResNet-50 encoder')
        self.P, self.B, self.dev = P, batch, device
        r = EncoderRoutes.from_env() if routes is None else routes
        self.routes = r = replace(r, stem=r.stem if 'stem.w4' in P else 'rowrun', block1=r.block1 and 1 in r.chain,
                                  front_split=r.front_split if r.front_split >= 1 and batch % r.front_split == 0 else 1)
        B, (H, W) = batch, in_hw
        self.H, self.W = H, W
        self.H2, self.W2 = _out(H, 7, 2, 3), _out(W, 7, 2, 3)
        self.H4, self.W4 = _out(self.H2, 3, 2, 1), _out(self.W2, 3, 2, 1)
        self.H8, self.W8 = _out(self.H4, 3, 2, 1), _out(self.W4, 3, 2, 1)
        self.H16, self.W16 = _out(self.H8, 3, 2, 1), _out(self.W8, 3, 2, 1)
        M4, M8, L = self.H4 * self.W4, self.H8 * self.W8, self.H16 * self.W16
        dt16 = P['stem.w'].dtype
        e = lambda *shape, dt=None: torch.empty(*shape, dtype=dt or dt16, device=device)  # noqa: E731
        self.img_in = e(B, 3, H, W, dt=F32)
        self._init_ptrs(B, device)
        # stem input: NHWC4 frames inside the zero border rmem_stem7x7s2 reads (zeroed once here, only the interior is ever written)
        if r.stem != 'rowrun':
            hp, wp = ops.stem_padded_size(H, W)
            self.img4 = torch.zeros(B, hp, wp, 4, dtype=dt16, device=device)
        else:      # the row-run form keeps the 8-channel layout
            self.img8 = e(B, H * W, 8)
        self.stem = None if r.stem == 'pool' else e(B, self.H2 * self.W2, 64)      # (stem + max-pool in one pass: the half-resolution map does not exist)
        self.pool = e(B, M4, 64)
        self.x4 = [e(B, M4, 256), e(B, M4, 256)]
        self.x8 = [e(B, M8, 512), e(B, M8, 512)]
        self.x16 = [e(B, L, 1024), e(B, L, 1024)]
        self.mid_a = e(B * M4 * 128)
        self.mid_b = e(B * M4 * 64)
        # layer 2's first conv1 output lives in its own buffer when the front is split: written per sub-batch while layer 1 still runs, its
        # 128-channel rows of sub-batch 0 would overlap the 64-channel rows of sub-batch 1 in mid_a
        self.mid_a128 = e(B * M4 * 128) if r.front_split > 1 else None
        self.conv_ws = torch.empty(16 * B * L * 256, dtype=F32, device=device)
        self._prog = None
        # the bottleneck blocks in order (nxt: the one after): geometry, weight keys (c3: conv3, or conv3 and the projection shortcut packed as
        # one GEMM) and the maps x (input), a, b (conv1's and conv2's outputs) and y as [image][elements] views of the whole-batch buffers
        rows = lambda t, n: t.reshape(-1)[:B * n].view(B, n)       # noqa: E731
        self.blocks, x, h, w, cin = [], rows(self.pool, M4 * 64), self.H4, self.W4, 64
        for li, (nblk, outs) in enumerate(zip(R50_BLOCKS, (self.x4, self.x8, self.x16)), start=1):
            for bi in range(nblk):
                p, planes, stride = f'encoder.layer{li}.{bi}', 64 * 2 ** (li - 1), R50_STRIDES[li - 1] if bi == 0 else 1
                ho, wo, dual = _out(h, 3, stride, 1), _out(w, 3, stride, 1), (p + '.c3ds.w') in P
                a = self.mid_a128 if (r.front_split > 1 and (li, bi) == (2, 0)) else self.mid_a
                self.blocks.append(SimpleNamespace(
                    li=li, bi=bi, c1=p + '.conv1', c2=p + '.conv2', c3=p + ('.c3ds' if dual else '.conv3'), planes=planes, cin=cin, stride=stride,
                    h=h, w=w, ho=ho, wo=wo, dual=dual, x=x, a=rows(a, h * w * planes), b=rows(self.mid_b, ho * wo * planes),
                    y=rows(outs[bi % 2], ho * wo * planes * 4), nxt=None))
                x, h, w, cin = self.blocks[-1].y, ho, wo, planes * 4
        for blk, nxt in zip(self.blocks, self.blocks[1:]):
            blk.nxt = nxt
        # stage outputs = the last block's buffer of every layer (block count - 1) % 2
        self.enc_out = (self.x4[(R50_BLOCKS[0] - 1) % 2], self.x8[(R50_BLOCKS[1] - 1) % 2], self.x16[(R50_BLOCKS[2] - 1) % 2])

    def _conv(self, nb, *a, **kw):
        return ops.conv2d(*a, ws=self.conv_ws, batch=nb, **kw)

    def _wb(self, key):
        return self.P[key + '.w'], self.P[key + '.b']

    def prog(self) -> list:
        if self._prog is None:
            steps = [(getattr(self, '_' + kind), self.blocks[i], flag) for kind, i, *flag in r50_steps(self.routes)]
            front = [s for s in steps if s[1].li == 1]
            o, nb = [], self.B // self.routes.front_split
            for b0 in range(0, self.B, nb):      # stem and layer 1, one sub-batch after the other
                o += self._stem(b0, nb) + [f(r, slice(b0, b0 + nb), nb, *flag) for f, r, flag in front]
            self._prog = o + [f(r, slice(0, self.B), self.B, *flag) for f, r, flag in steps[len(front):]]
        return self._prog

    def _stem(self, b0, nb) -> list:
        P, s, H, W = self.P, slice(b0, b0 + nb), self.H, self.W
        if self.routes.stem == 'rowrun':
            return [ops.image_ptrs_to_nhwc8(self.img_ptrs[b0:], self.img8[s], H=H, W=W, images=nb),
                    self._conv(nb, self.img8[s], P['stem.w'], P['stem.b'], self.stem[s], H=H, W=W, Cin=8, Cout=64, KH=7, KW=7, stride=2, pad=3, relu=True),
                    ops.maxpool3x3s2(self.stem[s], self.pool[s], H=self.H2, W=self.W2, C=64, images=nb)]
        q = [ops.image_ptrs_to_nhwc4p(self.img_ptrs[b0:], self.img4[s], H=H, W=W, images=nb)]
        if self.routes.stem == 'pool':     # stem + max-pool in one pass: the half-resolution map is never written
            return q + [ops.stem7x7s2_pool(self.img4[s], P['stem.w4'], P['stem.b'], self.pool[s], H=H, W=W, images=nb)]
        return q + [ops.stem7x7s2(self.img4[s], P['stem.w4'], P['stem.b'], self.stem[s], H=H, W=W, images=nb),
                    ops.maxpool3x3s2(self.stem[s], self.pool[s], H=self.H2, W=self.W2, C=64, images=nb)]

    # one launch per step kind of r50_steps: block r over the nb images s (a slice) of the batch
    def _block(self, r, s, nb, tail):
        # the tail: the next layer's first conv1 (128 planes) reads the y tile in place
        kw = dict(w1n=self.P[r.nxt.c1 + '.w'], bias1n=self.P[r.nxt.c1 + '.b'], a_next=r.nxt.a[s]) if tail else {}
        return ops.bneck_block64(r.x[s], *self._wb(r.c1), *self._wb(r.c2), *self._wb(r.c3), r.y[s], H=r.h, W=r.w, Cin=r.cin, images=nb, **kw)

    def _conv1(self, r, s, nb):
        return self._conv(nb, r.x[s], *self._wb(r.c1), r.a[s], H=r.h, W=r.w, Cin=r.cin, Cout=r.planes, relu=True)

    def _conv2(self, r, s, nb, direct):
        if direct:     # read in place from rows kept in LDS, weights in registers (bit-identical)
            return ops.conv3x3_direct(r.a[s], *self._wb(r.c2), r.b[s], H=r.h, W=r.w, C=r.planes, images=nb, relu=True)
        return self._conv(nb, r.a[s], *self._wb(r.c2), r.b[s], H=r.h, W=r.w, Cin=r.planes, Cout=r.planes, KH=3, KW=3, stride=r.stride, pad=1, relu=True)

    def _chain(self, r, s, nb):
        kw = dict(x2=r.x[s], H2=r.h, W2=r.w, Cin2=r.cin, stride2=r.stride) if r.dual else dict(residual=r.x[s])
        return ops.bneck_chain(r.b[s], *self._wb(r.c3), r.y[s], *self._wb(r.nxt.c1), r.nxt.a[s],
                               H=r.ho, W=r.wo, K1=r.planes, N2=r.nxt.planes, batch=nb, Cout=r.planes * 4, **kw)

    def _conv3(self, r, s, nb):
        if r.dual:     # conv3 + strided 1x1 shortcut as one GEMM: the shortcut tensor never exists
            return ops.conv1x1_dual(r.b[s], r.x[s], *self._wb(r.c3), r.y[s], H=r.ho, W=r.wo, Cin=r.planes, Cout=r.planes * 4,
                                    H2=r.h, W2=r.w, Cin2=r.cin, stride2=r.stride, relu=True, batch=nb)
        return self._conv(nb, r.b[s], *self._wb(r.c3), r.y[s], H=r.ho, W=r.wo, Cin=r.planes, Cout=r.planes * 4, residual=r.x[s], relu=True)


class SwinBatchEncoder(_PtrInput):
    """Swin-B (cfg 5; encoders/swin/swin_transformer.py:500-716) over B frames: patch embed (patch 4) + LN, 3 stages of
    (shifted-)window blocks with patch merging between them (500-545, 684-716), per-stage output norms.  One 720x1280 frame
    leaves only 3600 tokens for the 18 blocks of stage 3, so its linears are GEMMs of 3600 rows and its LayerNorms launches of
    3.7 MB; with B frames stacked as rows [frame][token] every linear and LayerNorm is ONE launch over B times the rows (weights
    are shared, rows independent); window attention and patch merging depend on the image geometry and take the frame as a grid
    dimension.  Interface of BatchEncoder (img_in, prog(), enc_out)."""

    def __init__(self, P: Dict[str, torch.Tensor], in_hw: Tuple[int, int], batch: int, device):
        if 'pe.w' not in P:
            raise ops.RmemError('SwinBatchEncoder covers the Swin-B encoder')
        self.P, self.B, self.dev = P, batch, device
        H, W = in_hw
        if H % 4 or W % 4:
            raise ops.RmemError('Swin-B path: network size must be a multiple of 4')
        self.H, self.W = H, W
        B = batch
        self.H4, self.W4 = H // 4, W // 4
        self.H8, self.W8 = (self.H4 + 1) // 2, (self.W4 + 1) // 2
        self.H16, self.W16 = (self.H8 + 1) // 2, (self.W8 + 1) // 2
        M4, M8, L = self.H4 * self.W4, self.H8 * self.W8, self.H16 * self.W16
        dt16 = P['proj.w'].dtype
        e = lambda *shape, dt=None: torch.empty(*shape, dtype=dt or dt16, device=device)  # noqa: E731
        self.img_in = e(B, 3, H, W, dt=F32)
        self._init_ptrs(B, device)
        self.img8 = e(B, H * W, 8)
        self.sx = e(B * M4, 128, dt=F32)            # fp32 residual stream of the current stage
        self.sln = e(B * M4, 128)
        self.sqkv = e(B * M4, 384)
        self.satt = e(B * M4, 128)
        self.smlp = e(B * M4, 512)
        self.smerge = e(B * M8, 512)
        self.enc_out = (e(B, M4, 128), e(B, M8, 256), e(B, L, 512))
        self.conv_ws = torch.empty(16 * B * L * 256, dtype=F32, device=device)
        self._prog = None

    def _lin(self, x, name, y, M, K, N, **kw):
        return ops.linear(x, self.P[name + '.w'], self.P[name + '.b'], y, M=M, K=K, N=N, ws=self.conv_ws, **kw)

    def prog(self) -> list:
        if self._prog is not None:
            return self._prog
        from .pack import SWIN_DEPTHS, SWIN_HEADS
        P, B, o = self.P, self.B, []
        o.append(self._input_op())
        h, w, C = self.H4, self.W4, 128
        x = self.sx.view(-1)
        o.append(ops.conv2d(self.img8, P['pe.w'], P['pe.b'], x[: B * h * w * C], H=self.H, W=self.W, Cin=8, Cout=C, KH=4, KW=4, stride=4,
                            batch=B))
        o.append(ops.layernorm(x, P['pe.ln.g'], P['pe.ln.b'], M=B * h * w, C=C, yf=x))
        for li, (depth, heads) in enumerate(zip(SWIN_DEPTHS, SWIN_HEADS)):
            M = h * w
            ln, qkv, att, mlp = self.sln.view(-1), self.sqkv.view(-1), self.satt.view(-1), self.smlp.view(-1)
            for b in range(depth):
                d = f'sw{li}.{b}'
                o.append(ops.layernorm(x, P[d + '.norm1.g'], P[d + '.norm1.b'], M=B * M, C=C, y=ln))
                o.append(self._lin(ln, d + '.qkv', qkv, B * M, C, 3 * C))
                o.append(ops.window_attn(qkv, P[d + '.qkv.b'], P[d + '.table'], att, H=h, W=w, C=C, heads=heads,
                                         shift=0 if b % 2 == 0 else 3, images=B))      # windows are cut per image
                o.append(self._lin(att, d + '.proj', x, B * M, C, C, residual=x))
                o.append(ops.layernorm(x, P[d + '.norm2.g'], P[d + '.norm2.b'], M=B * M, C=C, y=ln))
                o.append(self._lin(ln, d + '.fc1', mlp, B * M, C, 4 * C, relu=2))
                o.append(self._lin(mlp, d + '.fc2', x, B * M, 4 * C, C, residual=x))
            o.append(ops.layernorm(x, P[f'sw.norm{li}.g'], P[f'sw.norm{li}.b'], M=B * M, C=C, y=self.enc_out[li]))
            if li < len(SWIN_DEPTHS) - 1:
                mg = self.smerge.view(-1)
                h2, w2 = (h + 1) // 2, (w + 1) // 2
                o.append(ops.patch_merge_ln(x, P[f'sw{li}.merge.g'], P[f'sw{li}.merge.b'], mg, H=h, W=w, C=C, images=B))
                h, w = h2, w2
                o.append(ops.linear(mg, P[f'sw{li}.merge.w'], None, x, M=B * h * w, K=4 * C, N=2 * C, ws=self.conv_ws))
                C *= 2
        self._prog = o
        return o
