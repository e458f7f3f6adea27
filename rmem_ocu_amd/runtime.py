"""What the runtimes and the batch encoders share: model constants, the temporal-PE slot rule and the sine positional embedding.

The device state and the launch lists of a frame live in group_runtime.GroupRuntime (R50-AOTL, SwinB-AOTL) and
group_runtime_deaot.GroupRuntimeDeAOT (R50-DeAOTL): one class per model family, run with clips = 1 by the per-clip engines
(networks/engines/aot_engine.py) and with clips = B by GroupEngine.
"""
from __future__ import annotations

import os
from typing import List

import torch

BF16, F32 = torch.bfloat16, torch.float32
D_MODEL, HEADS, FFN = 256, 8, 1024
MAX_CHUNKS = 32
# key ranges of the one-frame (self / short-term) attention launches: 1 = every workgroup walks all keys and writes the
# normalised output itself (no partials, no combine launch)
PLAIN_CHUNKS = int(os.environ.get('RMEM_PLAIN_CHUNKS', 1))


def temporal_slots(T: int, n_slots: int = 4) -> List[int]:
    """Temporal-PE slot of each bank entry (layers/transformer.py:598-621).

    T <= 4: entry t uses slot t.  T > 4: the slots are flipped, nearest-resized to T
    (src = floor(dst * float32(4 / T))) and flipped back.
    """
    if T <= n_slots:
        return list(range(T))
    scale = torch.tensor(float(n_slots), dtype=F32) / torch.tensor(float(T), dtype=F32)
    out = []
    for t in range(T):
        src = int(torch.floor(torch.tensor(float(T - 1 - t), dtype=F32) * scale).item())
        out.append(n_slots - 1 - min(src, n_slots - 1))
    return out


def sine_pos_emb(h: int, w: int, c: int = D_MODEL) -> torch.Tensor:
    """2-D sine positional embedding [h*w, c] (layers/position.py:50-77: normalize=True,
    scale 2*pi, temperature 1e4, y half then x half); computed once per clip on the host."""
    nf = c // 2
    ys = torch.arange(h, dtype=F32)[:, None].expand(h, w)
    xs = torch.arange(w, dtype=F32)[None, :].expand(h, w)
    ys = ys / (ys[-1:, :] + 1e-6) * (2 * torch.pi)
    xs = xs / (xs[:, -1:] + 1e-6) * (2 * torch.pi)
    dim_t = 10000 ** (2 * torch.div(torch.arange(nf, dtype=F32), 2, rounding_mode='trunc') / nf)
    px, py = xs[:, :, None] / dim_t, ys[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).reshape(h * w, c).contiguous()


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1
