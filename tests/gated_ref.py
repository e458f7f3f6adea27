"""Plain dense float64 references of the DeAOT gated propagation attentions (rmem_ocu_amd/csrc/gated_attn.hip), a Python restatement
of the launch plan those kernels derive from the clip count, and the seeded inputs of the clip / half / dirty-workspace cases of
tests/test_hip_deaot_ops.py.  No GPU, no library: torch only (``device=`` evaluates the same torch code on a device).

tests/test_gated_ref_host.py checks, on the CPU, the references against the oracle, the plan of every case against the branch it is
meant to reach, and that the cases' inputs can see the bugs they exist for (a mutated reference moves by more than 5x the tolerance)."""
import math
from collections import namedtuple

import numpy as np
import torch

from test_hip_ops import seeded

F32, F64 = torch.float32, torch.float64
D_ATT, DV, KT, QT, CW, WIN_R, WIN = 128, 1024, 64, 128, 256, 7, 15
TOL = {torch.bfloat16: 2e-2, torch.float16: 4e-3}      # of max |ref| per clip: test_gated_attn_temporal_pe, test_mem_read_attn_fp16
MASS_TOL = 4e-3                                         # absolute, test_gated_attn_temporal_pe


def through(t, dt):
    """fp32 values rounded through the element type dt."""
    return t.to(dt).to(F32)


def _f64(t, device):
    return None if t is None else torch.as_tensor(t).to(device=device, dtype=F64)


# ------------------------------------------------------------------ references
def gated_ref(q, k, v, u, pe_cur=None, pe_mem=None, slots=None, *, keep=None, device=None):
    """(softmax((q + pe_cur)(k + pe_mem[slots])^T / sqrt(128)) v * u, mass [L, T]) in float64.  q [L, 128], k [T, Lk, 128],
    v [T, Lk, DV]; u [L, <= DV]: a narrower u is padded with ones (the layer-0 gate [SiLU(U) | ones]).
    keep (bool [T, Lk], mutation checks only): keys outside it do not exist."""
    device = q.device if device is None else device
    q, k, v, u, pe_cur, pe_mem = (_f64(t, device) for t in (q, k, v, u, pe_cur, pe_mem))
    T, Lk, _ = k.shape
    if pe_cur is not None:
        q = q + pe_cur
    if pe_mem is not None:
        k = k + pe_mem[torch.as_tensor(list(slots), device=device)][:, None, :]
    s = (q @ k.reshape(T * Lk, D_ATT).t()) / math.sqrt(D_ATT)
    if keep is not None:
        s = s.masked_fill(~keep.reshape(1, T * Lk).to(device), -math.inf)
    a = torch.softmax(s, dim=-1)
    out = a @ v.reshape(T * Lk, -1)
    if u.shape[1] < out.shape[1]:
        u = torch.cat([u, torch.ones(u.shape[0], out.shape[1] - u.shape[1], dtype=F64, device=device)], 1)
    return out * u, a.view(-1, T, Lk).sum(2)


def local_gated_ref(q, k, v, rel, u, H, W, *, radius=WIN_R, dx_shift=0, keep=None, device=None):
    """Dense L x L masked softmax of the 15x15 local attention in float64: key (y', x') is visible to query (y, x) iff |y' - y| <= 7
    and |x' - x| <= 7, with bias rel[q, (y' - y + 7) * 15 + (x' - x + 7)]; times u (padded with ones as in gated_ref).
    radius / dx_shift / keep (mutation checks only): a smaller window, the column offset of every key off by dx_shift, keys outside
    keep (bool [L]) do not exist."""
    device = q.device if device is None else device
    q, k, v, rel, u = (_f64(t, device) for t in (q, k, v, rel, u))
    L = H * W
    pos = torch.arange(L, device=device)
    y, x = pos // W, pos % W
    dy = y[None, :] - y[:, None]                        # [query, key]
    dx = x[None, :] - x[:, None] + dx_shift
    vis = (dy.abs() <= radius) & (dx.abs() <= radius)
    if keep is not None:
        vis = vis & keep.to(device)[None, :]
    idx = ((dy + WIN_R) * WIN + dx + WIN_R).clamp(0, WIN * WIN - 1)
    s = (q @ k.t()) / math.sqrt(D_ATT) + torch.gather(rel[:, :WIN * WIN], 1, idx)
    a = torch.softmax(s.masked_fill(~vis, -math.inf), dim=-1)
    out = a @ v
    if u.shape[1] < out.shape[1]:
        u = torch.cat([u, torch.ones(L, out.shape[1] - u.shape[1], dtype=F64, device=device)], 1)
    return out * u


def dwconv5x5_ref(x, w, H, W, *, device=None):
    """Depth-wise 5x5, zero padding 2, in float64: x [L, C] tokens of an H x W map, w [25, C] with tap dy * 5 + dx."""
    device = x.device if device is None else device
    x, w = _f64(x, device), _f64(w, device)
    C = x.shape[1]
    xp = torch.zeros(H + 4, W + 4, C, dtype=F64, device=device)
    xp[2:H + 2, 2:W + 2] = x.view(H, W, C)
    y = torch.zeros(H, W, C, dtype=F64, device=device)
    for dy in range(5):
        for dx in range(5):
            y += xp[dy:dy + H, dx:dx + W] * w[dy * 5 + dx]
    return y.view(H * W, C)


# ------------------------------------------------------------------ the launch plan, restated
Plan = namedtuple('Plan', 'nrows per groups key_tiles tiles_per_group empty_groups')


def plan_groups(Lq, frames, keys_per_frame, nclips, dv=DV):
    """plan() of gated_attn.hip: key groups (split-K slabs) = 256 / (query tiles * DV/256 * clips), at most 8 and at most the key tiles."""
    tiles = -(-Lq // QT) * (dv // CW) * nclips
    groups = 1 if tiles >= 256 else 256 // tiles
    return min(groups, 8, frames * -(-keys_per_frame // KT))


def _stream(groups, key_tiles):
    tpg = -(-key_tiles // groups)
    return tpg, sum(1 for g in range(groups) if g * tpg >= key_tiles)


def table_plan(Lq, rows, frames, keys_per_frame, nclips):
    """Chunk-table launch: rows = one clip's (slot, key_begin, key_count, pe_slot, t) rows; k_gp_pv cuts their key tiles, taken as one
    stream in table order, into `groups` equal ranges."""
    groups = plan_groups(Lq, frames, keys_per_frame, nclips)
    key_tiles = sum(-(-r[2] // KT) for r in rows)
    return Plan(len(rows), 0, groups, key_tiles, *_stream(groups, key_tiles))


def range_plan(L, want, nclips):
    """One key frame cut into `want` ranges that start on tile boundaries (rmem_gated_attn_clips without a table)."""
    per = -(-(-(-L // want)) // KT) * KT
    nrows = -(-L // per)
    groups = plan_groups(L, 1, L, nclips)
    key_tiles = sum(-(-min(per, L - r * per) // KT) for r in range(nrows))
    return Plan(nrows, per, groups, key_tiles, *_stream(groups, key_tiles))


def local_ranges(L, nclips):
    """Key ranges rmem_local_gated_attn_clips asks for (group_runtime_deaot.py uses the same rule for the self-attention's nchunks)."""
    tiles_q = -(-L // QT) * nclips
    return max(2, min(8, -(-448 // tiles_q)))


def local_plan(L, nclips):
    return range_plan(L, local_ranges(L, nclips), nclips)


def band_tiles(H, W, qt):
    """Key tiles [lo, hi) of the one key frame that a 15x15 window of query tile qt can touch (k_gp_scores<2, .> and k_gp_pv)."""
    L = H * W
    y0, y1 = qt * QT // W, min(qt * QT + QT - 1, L - 1) // W
    return max(0, (y0 - WIN_R) * W) // KT, -(-min(L, (y1 + WIN_R + 1) * W) // KT)


def frame_rows(T, L, splits, slots=None, pes=None, order=None):
    """Table rows of T frames of L keys, each cut into `splits` ranges on tile boundaries; frame t lives in bank slot slots[t], carries
    temporal slot pes[t]; frames appear in `order`."""
    per = -(-(-(-L // splits)) // KT) * KT
    rows = []
    for t in (range(T) if order is None else order):
        for kb in range(0, L, per):
            rows.append((t if slots is None else slots[t], kb, min(per, L - kb), -1 if pes is None else pes[t], t))
    return rows


# ------------------------------------------------------------------ the cases of tests/test_hip_deaot_ops.py
# groups / empty / nrows: what plan() gives at these shapes; test_gated_ref_host.py asserts them against the restatement above
LongCase = namedtuple('LongCase', 'name H W T clips splits ub groups key_tiles empty seed')
LONG_CASES = (
    LongCase('empty-groups', 11, 13, 3, 3, 1, False, 8, 9, 3, 7100),      # 8 groups over 9 key tiles: 2 2 2 2 1 0 0 0
    LongCase('mid-row-ranges', 15, 20, 5, 6, 2, True, 3, 25, 0, 7200),     # 192 + 108 keys per frame, ranges of 9 tiles; T > 4 slot table
    LongCase('one-group', 15, 20, 3, 11, 1, True, 1, 15, 0, 7300),         # the plan of the benchmark geometry
)
SelfCase = namedtuple('SelfCase', 'name H W clips nchunks nrows groups seed')
SELF_CASES = (
    SelfCase('three-groups', 11, 13, 3, 8, 3, 3, 7400),
    SelfCase('one-group', 11, 13, 17, 2, 2, 1, 7500),                      # rows of 128 + 15 keys
)
LocalCase = namedtuple('LocalCase', 'name H W clips ub nrows groups seed')
LOCAL_CASES = (
    LocalCase('small-ones', 11, 13, 3, False, 3, 3, 7600),
    LocalCase('small-ub', 11, 13, 3, True, 3, 3, 7610),
    LocalCase('7-ranges', 18, 23, 3, True, 7, 5, 7700),
    LocalCase('4-ranges', 18, 23, 32, True, 4, 1, 7800),
    LocalCase('2-ranges', 18, 23, 56, True, 2, 1, 7900),
)
QK_SCALE, SELF_SCALE, PE_SCALE, REL_SCALE = 1.5, 0.7, 0.5, 1.0


def long_slots(case):
    """Bank geometry of a long-term case: (bank slots, phys[clip][t] = the slot of clip's frame t, order[clip] = frame order of its
    table).  Two slots more than the clips need; the clips' frames are dealt over the slots by a fixed permutation."""
    S = case.clips * case.T + 2
    perm = np.random.Generator(np.random.PCG64([case.seed, 0xBA2C])).permutation(S).tolist()
    phys = [[perm[c * case.T + t] for t in range(case.T)] for c in range(case.clips)]
    order = [[(t + c) % case.T for t in range(case.T)] for c in range(case.clips)]
    return S, phys, order


def long_inputs(case, dt, clips=None):
    """q [clips, L, 128], k [clips, T, L, 128], v [clips, T, L, DV], u [clips, L, DV] (fp32, rounded through dt), pe_cur [128],
    pe_mem [4, 128] (fp32).  The values of clip c do not depend on how many clips are asked for."""
    n = case.clips if clips is None else clips
    L, T, s = case.H * case.W, case.T, case.seed
    return dict(q=through(seeded(s, (n, L, D_ATT), QK_SCALE), dt), k=through(seeded(s + 1, (n, T, L, D_ATT), QK_SCALE), dt),
                v=through(seeded(s + 2, (n, T, L, DV)), dt), u=through(seeded(s + 3, (n, L, DV)), dt),
                pe_cur=seeded(s + 4, (D_ATT,), PE_SCALE), pe_mem=seeded(s + 5, (4, D_ATT), PE_SCALE))


def self_inputs(case, dt, clips=None):
    """The fused [QK | V | U] rows of a self-attention case: [clips, L, 2176] fp32 rounded through dt (q = k columns 0..127)."""
    n = case.clips if clips is None else clips
    L = case.H * case.W
    x = seeded(case.seed, (n, L, D_ATT + 2 * DV))
    x[..., :D_ATT] *= SELF_SCALE
    return through(x, dt)


def local_inputs(case, dt, clips=None):
    """q, k [clips, L, 128], v, u [clips, L, DV] (fp32 rounded through dt), rel [clips, L, 225] fp32."""
    n = case.clips if clips is None else clips
    L, s = case.H * case.W, case.seed
    return dict(q=through(seeded(s, (n, L, D_ATT), QK_SCALE), dt), k=through(seeded(s + 1, (n, L, D_ATT), QK_SCALE), dt),
                v=through(seeded(s + 2, (n, L, DV)), dt), u=through(seeded(s + 3, (n, L, DV)), dt),
                rel=seeded(s + 4, (n, L, WIN * WIN), REL_SCALE))


def temporal_pe_inputs(T, L, dt):
    """The single-clip inputs of test_gated_attn_temporal_pe: q, k, v, u (fp32 rounded through dt), pe_cur, pe_mem."""
    return dict(q=through(seeded(10 + T, (L, D_ATT), 1.5), dt), k=through(seeded(20 + T, (T, L, D_ATT), 1.5), dt),
                v=through(seeded(30 + T, (T, L, DV)), dt), u=through(seeded(40 + T, (L, DV)), dt),
                pe_cur=seeded(50, (D_ATT,), 0.3), pe_mem=seeded(51, (4, D_ATT), 0.3))
