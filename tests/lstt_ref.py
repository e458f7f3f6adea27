"""Float64 references of the GroupRuntime stage programs (rmem_ocu_amd/group_runtime.py: prog_lstt propagate and reference mode,
prog_update, prog_project, prog_decode), the seeded state the stage tests start from, and the tolerances they are judged by.
No GPU, no library: torch and oracle/ref_cpu.py only.

Per stage there are three pieces:

  *_reference   the oracle itself (oracle.ref_cpu.lstt_block / ln / fpn_decode / OracleEngine._update_memories) in float64, one
                clip at a time with that clip's own bank order and length.  Intermediates the oracle does not return (k4, v4, tgt3,
                the FFN hidden, the decoder's stage outputs) are read off the oracle's own calls (``_taps``), not recomputed.
  *_restated    the same maths written out op by op.  With ``e16`` (``lstt_rounded`` and its kin are that form by name) it rounds
                through the element type at the store points of the unfused launch list; it exists only to measure how far rounding alone moves each output (``d_round``), never to
                judge the GPU.  With ``mut`` it is a WRONG reference: one deviation of the kind a launch list can have.
  *_MUTATIONS   the names of those deviations.

``tolerances(stage, dt, case=...)`` gives, per compared tensor, T = (3 * d_round emax, 2 * d_round erms), measured on that case's own
inputs from the references alone; tests/test_lstt_ref_host.py checks that every mutation moves some tensor by more than 3 * T and
that no T exceeds a third of the smallest mutation distance that counts on that tensor; tests/test_hip_lstt_stage.py imports the
same function."""
import contextlib
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

F32, F64 = torch.float32, torch.float64
C, HEADS, FFN, NL = 256, 8, 1024, 3
E16 = {'bf16': torch.bfloat16, 'fp16': torch.float16}
# Outputs stored in fp32 from operands that are exact on both sides (the projector's x) have d_round = 0.  What remains on the GPU
# is the fp32 accumulation of the longest dot product of these stages, K = 1024 terms: K * 2^-24 bounds it relative to the output's
# scale.  It is 50x under the bf16 and 7x under the fp16 rounding distances, so it decides nothing else.
F32_FLOOR = 1024 * 2.0 ** -24


def through(t, e16):
    """float64 values rounded through the element type (None: unchanged)."""
    return t if e16 is None else t.to(F32).to(e16).to(F64)


def metrics(got, ref):
    """(emax, erms) = (max |got - ref| / max |ref|, rms(got - ref) / rms(ref))."""
    got, ref = got.detach().to('cpu', F64), ref.detach().to('cpu', F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    return d.abs().max().item() / ref.abs().max().item(), math.sqrt((d * d).mean().item() / (ref * ref).mean().item())


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def geometry(hw):
    """ResNet-50 feature sizes of a network size: ((H4, W4), (H8, W8), (H16, W16))."""
    h, w = _out(hw[0], 7, 2, 3), _out(hw[1], 7, 2, 3)
    out = []
    for _ in range(3):
        h, w = _out(h, 3, 2, 1), _out(w, 3, 2, 1)
        out.append((h, w))
    return tuple(out)


# ------------------------------------------------------------------ weights
def stage_weights(state_dict, e16):
    """(The sine position embedding is not part of the state dict: stage_pos rounds it, as GroupRuntime.posb is rounded.)
    The oracle's weight dict (LSTT, decoder, projector; the encoder is not needed) in float64, with exactly the tensors that
    rmem_ocu_amd/pack.py stores in the element type rounded through it: the GEMM weights (linear and conv ``.weight`` of two or
    more dimensions).  Biases, norm gains, cur_pos_emb / mem_pos_emb, the GroupNorm parameters and the depth-wise 5x5 stay fp32."""
    w = {}
    for k, v in state_dict.items():
        if k.startswith('encoder.') or k.startswith('patch_wise_id_bank'):
            continue
        v = v.detach().to('cpu', F32)
        gemm = k.endswith('.weight') and v.dim() >= 2 and '.activation.conv.' not in k
        w[k] = through(v.to(F64), e16) if gemm else v.to(F64)
    return w


def stage_pos(size, e16):
    """Sine position embedding [L, 1, 256] of the 1/16 map, rounded through e16 as GroupRuntime.posb is."""
    return through(O.sine_pos_emb(*size).to(F64), e16)


# ------------------------------------------------------------------ seeded state
def seeded_lstt_state(B, L, S, seed=7):
    """The randn state of the chain identity tests (one generator; x, then per layer short_K, short_V, bank_K, bank_V), fp32."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    st = {'x': r(B * L, C), 'short_K': [], 'short_V': [], 'bank_K': [], 'bank_V': []}
    for _ in range(NL):
        st['short_K'].append(r(B * L, C)); st['short_V'].append(r(B * L, C))
        st['bank_K'].append(r(B * S, L, C)); st['bank_V'].append(r(B * S, L, C))
    return st


def fill_lstt_state(rt, seed=7):
    """Fill a GroupRuntime's residual stream, short-term memory and banks from seeded_lstt_state (the copy rounds to the buffers'
    element type).  Returns the fp32 state."""
    st = seeded_lstt_state(rt.B, rt.L, rt.S, seed)
    rt.x.copy_(st['x'])
    for i in range(NL):
        rt.short_K[i].copy_(st['short_K'][i]); rt.short_V[i].copy_(st['short_V'][i])
        rt.bank_K[i].copy_(st['bank_K'][i]); rt.bank_V[i].copy_(st['bank_V'][i])
    return st


def state64(st, e16):
    """What the runtime holds after fill_lstt_state, in float64: everything but the fp32 residual stream rounded through e16."""
    return {k: (v.to(F64) if k == 'x' else [through(t.to(F64), e16) for t in v]) for k, v in st.items()}


def seeded(seed, shape, scale=1.0):
    rng = np.random.Generator(np.random.PCG64([seed, 0x157A6E]))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


def shuffled_slots(B, T, S, seed):
    """Per clip T of the S bank slots in shuffled order, as after evictions."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x5107]))
    return [rng.permutation(S)[:T].tolist() for _ in range(B)]


# ------------------------------------------------------------------ the oracle, observed
class _TapF:
    """torch.nn.functional with relu and conv2d results recorded (fpn_decode calls them through the module's ``F``)."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, x):
        y = F.relu(x)
        self._rec['relu'].append(y)
        return y

    def conv2d(self, *a, **kw):
        y = F.conv2d(*a, **kw)
        self._rec['conv'].append(y)
        return y


@contextlib.contextmanager
def _taps():
    """Record what the oracle's own ln / mha / gn_gelu_dwconv / relu / conv2d calls return while it runs."""
    rec = {'ln': [], 'mha': [], 'ffn': [], 'relu': [], 'conv': []}
    ln0, mha0, gn0, f0 = O.ln, O.mha, O.gn_gelu_dwconv, O.F

    def ln(x, w, p):
        y = ln0(x, w, p)
        rec['ln'].append((p, y))
        return y

    def mha(*a, **kw):
        y = mha0(*a, **kw)
        rec['mha'].append(y[0])
        return y

    def gn(x, size, w, p):
        y = gn0(x, size, w, p)
        rec['ffn'].append((x, y))
        return y

    O.ln, O.mha, O.gn_gelu_dwconv, O.F = ln, mha, gn, _TapF(rec)
    try:
        yield rec
    finally:
        O.ln, O.mha, O.gn_gelu_dwconv, O.F = ln0, mha0, gn0, f0


def _temporal(w):
    return torch.cat((w['cur_pos_emb'], w['mem_pos_emb']), dim=0)


def _clip_inputs(st, c, i, L, S, slots, id_emb):
    rows = slice(c * L, (c + 1) * L)
    if id_emb is not None:
        return None, None, id_emb[rows]
    sl = [c * S + s for s in slots[c]]
    return (st['bank_K'][i][sl], st['bank_V'][i][sl]), (st['short_K'][i][rows], st['short_V'][i][rows]), None


def with_column_means(out):
    """Adds tgt3m_<i> = the column means of tgt3_<i> over all rows, a compared tensor of its own: rounding averages out of it, a
    per-column constant (the short-term projection's bias, 0.05 of max |tgt3|, which e16 rounding of single elements nearly
    hides) does not."""
    for i in range(NL):
        out[f'tgt3m_{i}'] = out[f'tgt3_{i}'].to(F64).mean(0)
    return out


def _collect(per_clip, masses, Tmax):
    out = with_column_means({k: torch.cat([pc[k] for pc in per_clip], 0) for k in per_clip[0]})
    if masses[0] is not None:
        L = masses[0].shape[0]
        m = torch.zeros(len(masses), L, Tmax, dtype=F64)
        for c, mc in enumerate(masses):
            m[c, :, :mc.shape[1]] = mc
        out['mass'] = m
    return out


def lstt_reference(w, pos, size, st, slots, S, id_emb=None):
    """The three LSTT blocks for B = len(slots) clips from explicit state, by the oracle, in float64.  st: x [B * L, 256], short_K/V
    per layer [B * L, 256], bank_K/V per layer [B * S, L, 256]; slots[c]: clip c's bank slots in logical order (its own T).
    id_emb [B * L, 256]: reference-frame mode (banks and short-term memory are outputs, not inputs).
    Returns {x<i>, cq<i>, cv<i>, k4_<i>, v4_<i>, tgt3_<i>, h1_<i>, h3_<i>, dec<i>: [B * L, .]} per block i, 'mass' [B, L, Tmax] of
    block 0 (propagate; frames a shorter bank does not have are zero), and in reference mode bank_K<i>, bank_V<i>, short_K<i>,
    short_V<i>."""
    B, L = len(slots), size[0] * size[1]
    per_clip, masses = [], []
    for c in range(B):
        x, o, mass = st['x'][c * L:(c + 1) * L].unsqueeze(1), {}, None
        for i in range(NL):
            bank, short, ide = _clip_inputs(st, c, i, L, S, slots, id_emb)
            long_mem = None if bank is None else [t.unsqueeze(2) for t in bank]
            short_mem = None if short is None else [t.unsqueeze(1) for t in short]
            with _taps() as rec:
                x, mem, record = O.lstt_block(x, w, f'LSTT.layers.{i}', long_mem, short_mem, None if ide is None else ide.unsqueeze(1),
                                              pos, size, _temporal(w), id_emb is None)
                dec = O.ln(x, w, f'LSTT.decoder_norms.{i}')
            norms = [y for p, y in rec['ln'] if p.endswith('.norm4')]
            o.update({f'x{i}': x, f'cq{i}': mem[0][0], f'cv{i}': mem[0][1], f'k4_{i}': norms[0], f'v4_{i}': norms[1],
                      f'tgt3_{i}': rec['mha'][2], f'h1_{i}': rec['ffn'][0][0], f'h3_{i}': rec['ffn'][0][1], f'dec{i}': dec})
            if id_emb is not None:
                o.update({f'bank_K{i}': mem[1][0][0], f'bank_V{i}': mem[1][1][0], f'short_K{i}': mem[2][0], f'short_V{i}': mem[2][1]})
            if i == 0:
                mass = record
        per_clip.append({k: v.squeeze(1) for k, v in o.items()})
        masses.append(mass)
    return _collect(per_clip, masses, max(len(s) for s in slots))


# ------------------------------------------------------------------ the restatement (rounding points, mutations)
LSTT_MUTATIONS = (
    'pe-slots-of-2-frames-as-for-T>4',      # temporal PE slot of a 2-frame bank taken by the flip / nearest rule
    'self-keys-without-pos',                # position embedding missing on the self-attention keys
    'k4-without-curr-K',                    # k4 = norm4(short_K)
    'v4-from-short-K',                      # v4 = norm4(short_K + curr_V)
    'tgt2-dropped',                         # the long-term read missing from the residual
    'short-proj-bias-missing',
    'gn-8-groups',                          # GroupNorm of the FFN hidden over 8 groups instead of 32
    'dw-transposed',                        # depth-wise 5x5 taps transposed
    'dec-norm-on-previous-block',           # decoder norm i applied to block i - 1's output
    'mass-over-clips',                      # mass = mean over the clips of head 0 instead of mean over the heads
    'residual-from-block-input',            # the long-term projection added to the block's input instead of the running x
    'curr-Q-from-x',                        # linear_Q reads the un-normed residual stream
)
LSTT_REF_MUTATIONS = (
    'bank-V-without-id',                    # linear_V(curr_V) without the identity embedding
    'short-V-without-id',
    'short-V-from-curr-V',                  # linear_VMem(curr_V + id) instead of tgt3 + id
    'short-memory-not-this-frame',          # norm4 sees curr_V twice instead of the frame's own bank value
    'self-keys-without-pos', 'tgt2-dropped', 'gn-8-groups', 'dw-transposed', 'dec-norm-on-previous-block',
)


def _ln(x, w, p):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w[p + '.weight'] + w[p + '.bias']


def _lin(x, w, p, bias=True):
    y = x @ w[p + '.weight'].t()
    return y + w[p + '.bias'] if bias else y


def _heads_attn(q, k, v):
    """([Lq, 256], probabilities [8, Lq, Lk]) of plain multi-head attention, scale 1 / sqrt(32)."""
    d = C // HEADS
    qh, kh, vh = (t.reshape(-1, HEADS, d).transpose(0, 1) for t in (q, k, v))
    a = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(d), dim=-1)
    return (a @ vh).transpose(0, 1).reshape(-1, C), a


def _ffn_act(h, size, w, p, groups=32, transposed=False):
    """GroupNorm(groups) -> exact GELU -> depth-wise 5x5 (zero padding 2) on tokens [L, 1024] of an H x W map."""
    H, W = size
    ch = h.shape[1]
    g = h.reshape(H * W, groups, ch // groups)
    mu = g.mean((0, 2), keepdim=True)
    var = ((g - mu) ** 2).mean((0, 2), keepdim=True)
    y = ((g - mu) / torch.sqrt(var + 1e-5)).reshape(H * W, ch) * w[p + '.gn.weight'] + w[p + '.gn.bias']
    y = 0.5 * y * (1 + torch.erf(y / math.sqrt(2.0)))
    k = w[p + '.conv.weight'][:, 0]                      # [1024, 5, 5]
    if transposed:
        k = k.transpose(1, 2)
    yp = torch.zeros(H + 4, W + 4, ch, dtype=F64)
    yp[2:H + 2, 2:W + 2] = y.view(H, W, ch)
    out = torch.zeros(H, W, ch, dtype=F64)
    for dy in range(5):
        for dx in range(5):
            out += yp[dy:dy + H, dx:dx + W] * k[:, dy, dx]
    return out.reshape(H * W, ch)


def _block(x, w, i, bank, short, ide, pos, size, r, m):
    """One LSTT block of one clip on [L, 256] tensors.  r rounds at the store points of the unfused launch list (prog_lstt): t1b,
    qkv, att, curr_V, curr_Q, k4, v4, tgt3, t3, h1, h3; the residual stream x is fp32 there and stays unrounded here."""
    p, L, o = f'LSTT.layers.{i}', x.shape[0], {}
    x_in = x
    # self-attention: qkv = t1b @ [Wq; Wk; Wv]^T + b + pos @ [Wq; Wk]^T  (GroupRuntime.pos_qk)
    t1 = r(_ln(x, w, p + '.norm1'))
    q = r(_lin(t1, w, p + '.self_attn.linear_Q') + _lin(pos, w, p + '.self_attn.linear_Q', False))
    k = _lin(t1, w, p + '.self_attn.linear_K')
    if m != 'self-keys-without-pos':
        k = k + _lin(pos, w, p + '.self_attn.linear_K', False)
    k, v = r(k), r(_lin(t1, w, p + '.self_attn.linear_V'))
    x = x + _lin(r(_heads_attn(q, k, v)[0]), w, p + '.self_attn.projection')
    # long-term read
    cv = r(_ln(x, w, p + '.norm2'))
    cq = r(_lin(x if m == 'curr-Q-from-x' else cv, w, p + '.linear_Q'))
    if ide is not None:
        new_v = r(_lin(cv if m == 'bank-V-without-id' else r(cv + ide), w, p + '.linear_V'))
        gK, gV, sk, sv = cq[None], new_v[None], cq, (cv if m == 'short-memory-not-this-frame' else new_v)
        o.update({f'bank_K{i}': cq, f'bank_V{i}': new_v})
    else:
        (gK, gV), (sk, sv) = bank, short
    T = gK.shape[0]
    pes = O.temporal_slots(T)
    if m == 'pe-slots-of-2-frames-as-for-T>4' and T == 2:
        pes = [3 - min(int(math.floor((T - 1 - t) * (4.0 / T))), 3) for t in range(T)]
    keys = (gK + w['mem_pos_emb'].reshape(4, C)[pes][:, None, :]).reshape(T * L, C)
    att, a = _heads_attn(cq + w['cur_pos_emb'].reshape(1, C), keys, gV.reshape(T * L, C))
    o['mass_heads'] = a.view(HEADS, L, T, L).sum(3)
    tgt2 = _lin(r(att), w, p + '.long_term_attn.projection')
    if m == 'tgt2-dropped':
        tgt2 = torch.zeros_like(tgt2)
    x = (x_in if m == 'residual-from-block-input' else x) + tgt2
    # short-term attention
    k4 = r(_ln(sk if m == 'k4-without-curr-K' else sk + cq, w, p + '.norm4'))
    v4 = r(_ln((sk if m == 'v4-from-short-K' else sv) + cv, w, p + '.norm4'))
    t3f = _lin(r(_heads_attn(cq, k4, v4)[0]), w, p + '.short_term_attn.projection', m != 'short-proj-bias-missing')
    tgt3 = r(t3f)                         # the e16 copy (y2); x takes the fp32 sum
    x = x + t3f
    if ide is not None:
        o[f'short_K{i}'] = r(_lin(tgt3, w, p + '.linear_QMem'))
        src = cv if m == 'short-V-from-curr-V' else tgt3
        o[f'short_V{i}'] = r(_lin(src if m == 'short-V-without-id' else r(src + ide), w, p + '.linear_VMem'))
    # feed-forward
    h1 = r(_lin(r(_ln(x, w, p + '.norm3')), w, p + '.linear1'))
    h3 = r(_ffn_act(h1, size, w, p + '.activation', 8 if m == 'gn-8-groups' else 32, m == 'dw-transposed'))
    x = x + _lin(h3, w, p + '.linear2')
    o.update({f'x{i}': x, f'cq{i}': cq, f'cv{i}': cv, f'k4_{i}': k4, f'v4_{i}': v4, f'tgt3_{i}': tgt3, f'h1_{i}': h1, f'h3_{i}': h3})
    return x, o


def lstt_restated(w, pos, size, st, slots, S, id_emb=None, e16=None, mut=None):
    """lstt_reference's arguments and results, op by op (see the module docstring): e16 rounds at the unfused list's store points
    (dec_in too), mut names one deviation of LSTT_MUTATIONS / LSTT_REF_MUTATIONS."""
    B, L = len(slots), size[0] * size[1]
    r = lambda t: through(t, e16)      # noqa: E731
    pos2, per_clip, heads = pos.reshape(L, C), [], []
    for c in range(B):
        x, o = st['x'][c * L:(c + 1) * L], {}
        for i in range(NL):
            bank, short, ide = _clip_inputs(st, c, i, L, S, slots, id_emb)
            x_prev = x
            x, ob = _block(x, w, i, bank, short, ide, pos2, size, r, mut)
            mh = ob.pop('mass_heads')
            if i == 0:
                heads.append(mh)
            o.update(ob)
            o[f'dec{i}'] = r(_ln(x_prev if mut == 'dec-norm-on-previous-block' else x, w, f'LSTT.decoder_norms.{i}'))
        per_clip.append(o)
    Tmax = max(len(s) for s in slots)
    if id_emb is not None:
        masses = [None] * B
    elif mut == 'mass-over-clips':
        pad = torch.zeros(B, L, Tmax, dtype=F64)
        for c, mh in enumerate(heads):
            pad[c, :, :mh.shape[2]] = mh[0]
        masses = [pad.mean(0)] * B
    else:
        masses = [mh.mean(0) for mh in heads]
    return _collect(per_clip, masses, Tmax)


# ------------------------------------------------------------------ prog_update
UPDATE_KEYS = ('tgt3', 'curr_V', 'curr_Q')
UPDATE_MUTATIONS = (
    'short-V-without-id',
    'new-V-from-tgt3',                      # linear_V(tgt3 + id)
    'short-K-through-VMem',                 # linear_VMem's weights on the short-term keys
    'bank-K-from-curr-V',                   # curr_V scattered as the key entry
    'layer-weights-rotated',                # the grouped linears pair layer i with layer i + 1's weights
)


def update_inputs(B, L, e16, seed=2100):
    """Seeded tgt3 / curr_V / curr_Q per layer and id_emb, [B * L, 256] float64 rounded through e16."""
    st = {k: [through(seeded(seed + 10 * j + i, (B * L, C)).to(F64), e16) for i in range(NL)] for j, k in enumerate(UPDATE_KEYS)}
    st['id_emb'] = through(seeded(seed + 99, (B * L, C)).to(F64), e16)
    return st


def update_reference(w, st, B, L):
    """prog_update(append=True) by the oracle: OracleEngine._update_memories on curr_mem = [curr_K, curr_V] and lstt_short =
    [linear_QMem(tgt3), tgt3] (the latter as lstt_block leaves them, transformer.py:675-676) with update_long.  Returns short_K<i>,
    short_V<i>, new_V<i> (the bank's value entry) and bank_K<i> (= curr_K), [B * L, 256]."""
    lbc = lambda t: t.view(B, L, C).transpose(0, 1)      # noqa: E731
    eng = O.OracleEngine(w, former_len=1, latter_len=1 << 20)
    eng.curr_mem = [[lbc(st['curr_Q'][i]), lbc(st['curr_V'][i])] for i in range(NL)]
    eng.lstt_short = [[F.linear(lbc(st['tgt3'][i]), w[f'LSTT.layers.{i}.linear_QMem.weight'], w[f'LSTT.layers.{i}.linear_QMem.bias']),
                       lbc(st['tgt3'][i])] for i in range(NL)]
    eng.long_mem = [[torch.zeros(0, L, B, C, dtype=F64), torch.zeros(0, L, B, C, dtype=F64)] for _ in range(NL)]
    eng.pred_id_logits, eng.enc_size_2d = torch.zeros(1, 11, 2, 2, dtype=F64), (2, 2)
    eng._update_memories(lbc(st['id_emb']), True)
    back = lambda t: t.transpose(0, 1).reshape(B * L, C)      # noqa: E731
    out = {}
    for i in range(NL):
        out.update({f'short_K{i}': back(eng.short_mem[i][0]), f'short_V{i}': back(eng.short_mem[i][1]),
                    f'bank_K{i}': back(eng.long_mem[i][0][-1]), f'new_V{i}': back(eng.long_mem[i][1][-1])})
    return out


def update_restated(w, st, B, L, e16=None, mut=None):
    """The launch list of prog_update, rounding at tmpA, tmpB and the three linears' outputs."""
    r = lambda t: through(t, e16)      # noqa: E731
    out = {}
    for i in range(NL):
        p = f'LSTT.layers.{(i + 1) % NL if mut == "layer-weights-rotated" else i}'
        tgt3, cv, ide = st['tgt3'][i], st['curr_V'][i], st['id_emb']
        out[f'short_K{i}'] = r(_lin(tgt3, w, p + ('.linear_VMem' if mut == 'short-K-through-VMem' else '.linear_QMem')))
        out[f'short_V{i}'] = r(_lin(tgt3 if mut == 'short-V-without-id' else r(tgt3 + ide), w, p + '.linear_VMem'))
        out[f'new_V{i}'] = r(_lin(r((tgt3 if mut == 'new-V-from-tgt3' else cv) + ide), w, p + '.linear_V'))
        out[f'bank_K{i}'] = cv if mut == 'bank-K-from-curr-V' else st['curr_Q'][i]
    return out


# ------------------------------------------------------------------ prog_project
PROJECT_MUTATIONS = ('bias-missing', 'relu', 'dec-copy-of-previous-row')


def project_reference(w, enc3):
    """encoder_projector (oracle.encode_image's last line) on enc3 [R, 1024]: x [R, 256] and its copy for dec_in[:, :256]."""
    x = F.conv2d(enc3.t()[None, :, :, None], w['encoder_projector.weight'], w['encoder_projector.bias'])[0, :, :, 0].t()
    return {'x': x, 'dec0': x}


def project_restated(w, enc3, e16=None, mut=None):
    x = enc3 @ w['encoder_projector.weight'].reshape(C, -1).t()
    if mut != 'bias-missing':
        x = x + w['encoder_projector.bias']
    if mut == 'relu':
        x = x.clamp(min=0)
    return {'x': x, 'dec0': through(x.roll(1, 0) if mut == 'dec-copy-of-previous-row' else x, e16)}


# ------------------------------------------------------------------ prog_decode
# The two adapters have different channel counts, so they cannot literally trade places; what a launch list can get wrong about
# them is where they sit relative to the resize (the fused route resizes the residual inside the adapter's GEMM): with
# 'adapters-8x-4x-before-the-resize' the sum adapter(shortcut) + x is formed at the coarse size and resized as a whole, or they
# are dropped.  'dec-in-blocks-swapped' is the assembly of dec_in itself.
DECODE_MUTATIONS = (
    'align-corners-inverted',
    'adapter-8x-missing', 'adapter-4x-missing', 'adapter-16x-missing',
    'adapters-8x-4x-before-the-resize',     # adapter(shortcut) resized along with x: the sum formed at the coarse size's order
    'dec-in-blocks-swapped',                # LSTT blocks 1 and 2 trade places in the concat
    'gn-32-groups',
    'relu-missing-after-conv-in',
    'residual-from-conv-in',                # the 16x stage's sum feeds the 8x stage's residual without conv_16x + GN + ReLU
)
DECODE_ROUTES = {'default': (), 'no_upfuse': ('up',), 'direct128': (), 'no_headfuse': ('head',)}
DECODE_ENV = {'default': {}, 'no_upfuse': {'RMEM_NO_UPFUSE': '1'}, 'direct128': {'RMEM_DIRECT_CONV3_128': '1'},
              'no_headfuse': {'RMEM_NO_HEADFUSE': '1'}}


def decode_inputs(B, hw, e16, seed=3100):
    """Seeded encoder outputs (enc1 [B * M4, 256], enc2 [B * M8, 512], enc3 [B * L, 1024]; non-negative like the ReLU outputs they
    stand for) and dec_in [B * L, 1024], float64 rounded through e16."""
    (h4, w4), (h8, w8), (h16, w16) = geometry(hw)
    enc = tuple(through(seeded(seed + j, (B * h * wd, ch)).abs().to(F64), e16)
                for j, (h, wd, ch) in enumerate(((h4, w4, 256), (h8, w8, 512), (h16, w16, 1024))))
    return enc, through(seeded(seed + 9, (B * h16 * w16, 4 * C)).to(F64), e16)


def _nchw(t, B, size):
    return t.reshape(B, size[0], size[1], -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def decode_reference(w, enc, dec_in, B, hw, align):
    """fpn_decode on dec_in's four 256-column blocks and the encoder outputs.  Returns logits [B * M4, 11] and the stage outputs
    d16a (ReLU(GN(conv_16x))), d8d (ReLU(GN(conv_8x))) and d4a (conv_4x before its norm), rows [image][y][x]."""
    s4, s8, s16 = geometry(hw)
    ins = [_nchw(dec_in[:, k * C:(k + 1) * C], B, s16) for k in range(4)]
    xs = [_nchw(enc[0], B, s4), _nchw(enc[1], B, s8), _nchw(enc[2], B, s16), None]
    with _taps() as rec:
        logits = O.fpn_decode(ins, xs, w, align)
    return {'logits': _rows(logits), 'd16a': _rows(rec['relu'][1]), 'd8d': _rows(rec['relu'][2]), 'd4a': _rows(rec['conv'][6])}


def decode_restated(w, enc, dec_in, B, hw, align, e16=None, mut=None, route=()):
    """prog_decode's launch list: every buffer it stores in the element type is rounded (d16a/b, d8b/c/d, d4b/a); route adds the
    stores of the unfused variants: 'up' the resized maps (group_runtime.py:409, 421: ops.bilinear into d8a / d4a), 'head' the
    normed 1/4 map (group_runtime.py:429: groupnorm into d4b)."""
    r = lambda t: through(t, e16)      # noqa: E731
    s4, s8, s16 = geometry(hw)
    if mut == 'align-corners-inverted':
        align = not align
    groups = 32 if mut == 'gn-32-groups' else 8
    conv = lambda x, p, k: F.conv2d(x, w[p + '.conv.weight'], w[p + '.conv.bias'], padding=k // 2)      # noqa: E731
    gn = lambda x, p: F.relu(F.group_norm(x, groups, w[p + '.gn.weight'], w[p + '.gn.bias'], 1e-5))      # noqa: E731
    ad = lambda x, p: F.conv2d(x, w[p + '.weight'], w[p + '.bias'])      # noqa: E731
    up = lambda x, size: F.interpolate(x, size=size, mode='bilinear', align_corners=align)      # noqa: E731
    e1, e2, e3 = _nchw(enc[0], B, s4), _nchw(enc[1], B, s8), _nchw(enc[2], B, s16)
    order = (0, 2, 1, 3) if mut == 'dec-in-blocks-swapped' else (0, 1, 2, 3)
    x = r(conv(torch.cat([_nchw(dec_in[:, k * C:(k + 1) * C], B, s16) for k in order], 1), 'decoder.conv_in', 1))
    x = r(x if mut == 'relu-missing-after-conv-in' else gn(x, 'decoder.conv_in'))
    x0 = x = r(x if mut == 'adapter-16x-missing' else ad(e3, 'decoder.adapter_16x') + x)
    d16a = r(gn(r(conv(x, 'decoder.conv_16x', 3)), 'decoder.conv_16x'))
    x = x0 if mut == 'residual-from-conv-in' else d16a

    def stage(x, e, size, name):
        a = ad(e, f'decoder.adapter_{name}')
        if mut == f'adapter-{name}-missing':
            a = torch.zeros_like(a)
        if mut == 'adapters-8x-4x-before-the-resize':     # the shortcut's sum goes through a down-and-up resize with x
            a = up(F.interpolate(a, size=x.shape[-2:], mode='bilinear', align_corners=align), size)
        x = up(x, size)
        return r(a + (r(x) if 'up' in route else x))

    x = stage(x, e2, s8, '8x')
    d8d = r(gn(r(conv(x, 'decoder.conv_8x', 3)), 'decoder.conv_8x'))
    x = stage(d8d, e1, s4, '4x')
    d4a = r(conv(x, 'decoder.conv_4x', 3))
    x = gn(d4a, 'decoder.conv_4x')
    logits = F.conv2d(r(x) if 'head' in route else x, w['decoder.conv_out.weight'], w['decoder.conv_out.bias'])
    return {'logits': _rows(logits), 'd16a': _rows(d16a), 'd8d': _rows(d8d), 'd4a': _rows(d4a)}


# ------------------------------------------------------------------ the names the rounding emulation goes by
def lstt_rounded(w, pos, size, st, slots, S, id_emb=None, *, e16):
    """lstt_restated with rounding through e16 at the unfused list's store points: what d_round is measured with."""
    return lstt_restated(w, pos, size, st, slots, S, id_emb, e16=e16)


def update_rounded(w, st, B, L, *, e16):
    return update_restated(w, st, B, L, e16=e16)


def project_rounded(w, enc3, *, e16):
    return project_restated(w, enc3, e16=e16)


def decode_rounded(w, enc, dec_in, B, hw, align, *, e16, route=()):
    return decode_restated(w, enc, dec_in, B, hw, align, e16=e16, route=route)


# ------------------------------------------------------------------ cases, d_round, tolerances, mutation distances
CANON_SLOTS = [[0], [2, 1, 3, 0, 4], [1, 3]]      # banks of 1, 5 and 2 frames: every temporal-slot rule, a padded table
STAGES = ('lstt', 'lstt_ref', 'update', 'project', 'decode')
MUTATIONS = {'lstt': LSTT_MUTATIONS, 'lstt_ref': LSTT_REF_MUTATIONS, 'update': UPDATE_MUTATIONS, 'project': PROJECT_MUTATIONS,
             'decode': DECODE_MUTATIONS}
CLIPS, DECODE_IMAGES = 3, 2


@functools.lru_cache(maxsize=None)
def weights(dt):
    from rmem_ocu_amd.weights import synth_state_dict
    return stage_weights(synth_state_dict(0), E16[dt])


def ref_inputs(B, L, e16, seed=1100):
    """Reference-frame mode: seeded x (fp32) and id_emb (e16) [B * L, 256]."""
    return {'x': seeded(seed, (B * L, C)).to(F64)}, through(seeded(seed + 1, (B * L, C)).to(F64), e16)


def project_inputs(B, L, e16, seed=4200):
    """A seeded encoder output [B * L, 1024], non-negative, rounded through e16."""
    return through(seeded(seed, (B * L, 1024)).abs().to(F64), e16)


# The cases of tests/test_hip_lstt_stage.py, per stage.  Every case is judged by tolerances measured on ITS OWN inputs (d_round is
# the distance between the rounded restatement and the reference on the same inputs): geometry, seeds and, for the mass, which is
# relative to its largest element (1 / T-ish; exactly 1 with a 1-frame bank in the group), the banks' lengths all move it a little.
# propagate: (network size, bank slots S, slots per clip); reference frame, update, project: network size; decode: (size, align).
def _lstt_cases():
    out = {}
    for hw in ((161, 193), (129, 257)):
        tok = geometry(hw)[2][0] * geometry(hw)[2][1]
        for T in (1, 2, 5, 8):
            S = max(5, T + 1)
            out[f'{tok}tok/T{T}'] = (hw, S, tuple(tuple(s) for s in shuffled_slots(CLIPS, T, S, 100 + T)))
    out['banks-2-1-2'] = ((161, 193), 5, ((1, 3), (2,), (1, 3)))
    out['banks-1-5-2'] = ((161, 193), 5, tuple(tuple(s) for s in CANON_SLOTS))
    return out


LSTT_CASES = _lstt_cases()
CASES = {'lstt': LSTT_CASES,
         'lstt_ref': {'143tok': (161, 193), '153tok': (129, 257)},
         'update': {'143tok': (161, 193)},
         'project': {'143tok': (161, 193), '153tok': (129, 257)},
         'decode': {'161x193': ((161, 193), True), '129x257': ((129, 257), True), '160x192': ((160, 192), False)}}
# the case the mutation distances are measured on
CANON = {'lstt': 'banks-1-5-2', 'lstt_ref': '143tok', 'update': '143tok', 'project': '143tok', 'decode': '161x193'}
_FUNCS = {'lstt': (lstt_reference, lstt_rounded, lstt_restated), 'lstt_ref': (lstt_reference, lstt_rounded, lstt_restated),
          'update': (update_reference, update_rounded, update_restated), 'project': (project_reference, project_rounded, project_restated),
          'decode': (decode_reference, decode_rounded, decode_restated)}


@functools.lru_cache(maxsize=None)
def stage_args(stage, dt, case):
    """The arguments of a stage's reference (= of its restatement) for a case: the seeded inputs the GPU test loads, in float64."""
    e16, w, spec = E16[dt], weights(dt), CASES[stage][case]
    if stage == 'lstt':
        hw, S, slots = spec
        size, slots = geometry(hw)[2], [list(s) for s in slots]
        return (w, stage_pos(size, e16), size, state64(seeded_lstt_state(len(slots), size[0] * size[1], S), e16), slots, S)
    if stage == 'decode':
        hw, align = spec
        enc, dec_in = decode_inputs(DECODE_IMAGES, hw, e16)
        return (w, enc, dec_in, DECODE_IMAGES, hw, align)
    size = geometry(spec)[2]
    L = size[0] * size[1]
    if stage == 'lstt_ref':
        st, ide = ref_inputs(CLIPS, L, e16)
        return (w, stage_pos(size, e16), size, st, [[0]] * CLIPS, 1, ide)
    if stage == 'update':
        return (w, update_inputs(CLIPS, L, e16), CLIPS, L)
    return (w, project_inputs(CLIPS, L, e16))


@functools.lru_cache(maxsize=None)
def stage_case(stage, dt, case, route=()):
    """(reference, rounded restatement) of a case; route: the decoder's extra store points (DECODE_ROUTES)."""
    ref_fn, rounded_fn, _ = _FUNCS[stage]
    args = stage_args(stage, dt, case)
    kw = {'route': route} if stage == 'decode' else {}
    return reference_case(stage, dt, case), rounded_fn(*args, e16=E16[dt], **kw)


@functools.lru_cache(maxsize=None)
def reference_case(stage, dt, case):
    return _FUNCS[stage][0](*stage_args(stage, dt, case))


def lstt_case(dt, case):
    return stage_case('lstt', dt, case)


def _canon(stage, dt, route=()):
    """(reference, rounded restatement, mutated(m): the restatement without rounding and with mutation m) on the stage's canonical case."""
    args = stage_args(stage, dt, CANON[stage])
    return (*stage_case(stage, dt, CANON[stage], route), lambda m: _FUNCS[stage][2](*args, mut=m))


@functools.lru_cache(maxsize=None)
def d_round(stage, dt, route=(), case=None):
    """{tensor: (emax, erms)} between the rounded restatement and the reference on the inputs of ``case`` (default: the stage's
    canonical case, on which the mutation distances are measured too)."""
    ref, rounded = stage_case(stage, dt, case or CANON[stage], route)
    return {k: metrics(rounded[k], ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def tolerances(stage, dt, route=(), case=None):
    """{tensor: (T for emax, T for erms)} = (3 * d_round, 2 * d_round_rms) of that case, not below the fp32 floor.  The GPU tests
    and the host tests both take their tolerances from here; every GPU test passes its own case."""
    return {k: (max(3 * a, F32_FLOOR), max(2 * b, F32_FLOOR)) for k, (a, b) in d_round(stage, dt, route, case).items()}


@functools.lru_cache(maxsize=None)
def mutation_distances(stage, dt):
    """{mutation: {tensor: (emax, erms)}} of every wrong reference against the reference, on the stage's canonical case."""
    ref, _, mutated = _canon(stage, dt)
    out = {}
    for m in MUTATIONS[stage]:
        got = mutated(m)
        out[m] = {k: metrics(got[k], ref[k]) for k in ref}
    return out


# what the GPU keeps after prog_lstt: per-block buffers of every block, shared buffers of the last block only
def lstt_compared(ref_mode=False):
    keys = ['x2', 'k4_2', 'v4_2', 'h1_2', 'h3_2'] + [f'{n}{i}' for i in range(NL) for n in ('cq', 'cv', 'tgt3_', 'tgt3m_', 'dec')]
    if ref_mode:
        return keys + [f'{n}{i}' for i in range(NL) for n in ('bank_K', 'bank_V', 'short_K', 'short_V')]
    return keys + ['mass']
