"""Host side of the batch ResNet-50 encoder (no GPU, no library): EncoderRoutes.from_env, the plan r50_steps, and the launch list
BatchEncoder builds from it with the ops.* constructors replaced by recorders -- names and counts per route as the list before the
plan produced them, every convolution produced once, and every map read from the launch that was meant to write it."""
import pytest
import torch

from rmem_ocu_amd.encoder_batch import EncoderRoutes, r50_steps

R = EncoderRoutes
# route: (routes, launches at B = 2, rmem_bneck_block64, rmem_bneck_chain, rmem_conv3x3_direct, rmem_conv1x1_dual_nhwc, rmem_conv2d_nhwc)
TABLE = {
    'default': (R(), 30, 3, 4, 0, 1, 20),
    'block1 off': (R(block1=False), 34, 0, 7, 3, 1, 21),
    'layer-2 chain off': (R(chain=(1,)), 34, 3, 0, 0, 2, 27),
    'all chains off': (R(block1=False, chain=()), 41, 0, 0, 3, 3, 33),
    'direct3 off': (R(direct3=()), 30, 3, 4, 0, 1, 20),
    'block1 off, direct3 off': (R(block1=False, direct3=()), 34, 0, 7, 0, 1, 24),
    'direct3 64 and 128': (R(direct3=(64, 128)), 30, 3, 4, 3, 1, 17),
    'stem direct': (R(stem='direct'), 31, 3, 4, 0, 1, 20),
    'stem rowrun': (R(stem='rowrun'), 31, 3, 4, 0, 1, 21),                  # one conv2d is the stem
    'front_split 2': (R(front_split=2), 35, 6, 4, 0, 1, 20),
    'front_split 2, block1 off': (R(front_split=2, block1=False), 43, 0, 10, 6, 1, 22),
    'front_split 3': (R(front_split=3), 30, 3, 4, 0, 1, 20),                 # 3 does not divide B = 2: one batch
}
STEM_LAUNCHES = {'pool': 2, 'direct': 3, 'rowrun': 3}
N1, NBLOCKS = 3, 13                                        # ResNet-50: blocks of layer 1, of layers 1-3


# ---- EncoderRoutes.from_env ----

def test_from_env_defaults():
    assert R.from_env({}) == R() == R(stem='pool', front_split=1, block1=True, chain=(1, 2), direct3=(64,))


@pytest.mark.parametrize('env,want', [
    ({'RMEM_STEM': 'pool'}, R()),
    ({'RMEM_STEM': 'rowrun'}, R(stem='rowrun')),
    ({'RMEM_STEM': 'direct'}, R(stem='direct')),
    ({'RMEM_STEM': 'bogus'}, R(stem='direct')),                               # any other value
    ({'RMEM_STEM': ''}, R(stem='direct')),
    ({'RMEM_ENC_FRONT_SPLIT': '2'}, R(front_split=2)),
    ({'RMEM_ENC_FRONT_SPLIT': ' 4 '}, R(front_split=4)),                     # int() strips
    ({'RMEM_ENC_FRONT_SPLIT': '0'}, R(front_split=0)),                        # kept as requested: the encoder falls back to 1
    ({'RMEM_ENC_FRONT_SPLIT': '-2'}, R(front_split=-2)),
    ({'RMEM_NO_BNECK_CHAIN': '1'}, R(block1=False, chain=())),
    ({'RMEM_NO_BNECK_CHAIN': '1', 'RMEM_NO_BNECK_BLOCK': '0', 'RMEM_NO_BNECK_CHAIN2': '0'}, R(block1=False, chain=())),
    ({'RMEM_NO_BNECK_CHAIN': '0'}, R()),
    ({'RMEM_NO_BNECK_CHAIN': 'yes'}, R()),                                    # only '1' switches
    ({'RMEM_NO_BNECK_BLOCK': '1'}, R(block1=False)),
    ({'RMEM_NO_BNECK_BLOCK': '0'}, R()),
    ({'RMEM_NO_BNECK_BLOCK': 'true'}, R()),
    ({'RMEM_NO_BNECK_CHAIN2': '1'}, R(chain=(1,))),
    ({'RMEM_NO_BNECK_CHAIN2': '0'}, R()),                                     # '0' means enabled
    ({'RMEM_NO_BNECK_CHAIN2': ''}, R()),
    ({'RMEM_NO_BNECK_CHAIN2': '1', 'RMEM_NO_BNECK_BLOCK': '1'}, R(block1=False, chain=(1,))),
    ({'RMEM_NO_DIRECT_CONV3': '1'}, R(direct3=())),
    ({'RMEM_NO_DIRECT_CONV3': '128'}, R()),                                   # not '1'
    ({'RMEM_DIRECT_CONV3_128': '1'}, R(direct3=(64, 128))),
    ({'RMEM_DIRECT_CONV3_128': '0'}, R()),
    ({'RMEM_NO_DIRECT_CONV3': '1', 'RMEM_DIRECT_CONV3_128': '1'}, R(direct3=())),      # off wins
    ({'RMEM_NO_UPFUSE': '1', 'RMEM_NO_CHAIN': '1'}, R()),                     # the group runtime's switches are not the encoder's
])
def test_from_env_parse_rules(env, want):
    assert R.from_env(env) == want


@pytest.mark.parametrize('bad', ['two', '', '1.5'])
def test_from_env_bad_front_split_raises(bad):
    with pytest.raises(ValueError):
        R.from_env({'RMEM_ENC_FRONT_SPLIT': bad})


def test_from_env_reads_the_process_environment_by_default(monkeypatch):
    for k in ('RMEM_STEM', 'RMEM_ENC_FRONT_SPLIT', 'RMEM_NO_BNECK_CHAIN', 'RMEM_NO_BNECK_BLOCK', 'RMEM_NO_DIRECT_CONV3', 'RMEM_DIRECT_CONV3_128'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RMEM_NO_BNECK_CHAIN2', '1')
    assert R.from_env() == R(chain=(1,))


def test_routes_are_a_value():
    with pytest.raises(Exception):
        R().block1 = False
    assert hash(R(chain=(1,))) == hash(R(chain=(1,))) and R(chain=(1,)) != R()


# ---- the plan ----

def _step_name(step):
    """The library entry a step of the plan becomes; the first block of a layer has the projection shortcut (conv1x1_dual)."""
    kind, i = step[0], step[1]
    if kind == 'block':
        return 'rmem_bneck_block64'
    if kind == 'chain':
        return 'rmem_bneck_chain'
    if kind == 'conv2' and step[2]:
        return 'rmem_conv3x3_direct'
    if kind == 'conv3' and i in (0, 3, 7):
        return 'rmem_conv1x1_dual_nhwc'
    assert kind in ('conv1', 'conv2', 'conv3')
    return 'rmem_conv2d_nhwc'


@pytest.mark.parametrize('route', list(TABLE))
def test_plan_counts_per_route(route):
    """Steps of the bottleneck stack = the launch total minus the stem's launches, the front (layer 1) once per sub-batch."""
    routes, launches, nblock, nchain, ndirect, ndual, nconv = TABLE[route]
    steps = r50_steps(routes)
    split = routes.front_split if 2 % routes.front_split == 0 else 1           # B = 2
    front = [s for s in steps if s[1] < N1]
    assert steps[:len(front)] == front                                         # layer 1 comes first, whole
    names = [_step_name(s) for s in front] * split + [_step_name(s) for s in steps[len(front):]]
    assert len(names) == launches - STEM_LAUNCHES[routes.stem] * split
    got = tuple(names.count(n) for n in ('rmem_bneck_block64', 'rmem_bneck_chain', 'rmem_conv3x3_direct', 'rmem_conv1x1_dual_nhwc'))
    assert got == (nblock, nchain, ndirect, ndual)
    assert names.count('rmem_conv2d_nhwc') == nconv - (1 if routes.stem == 'rowrun' else 0)


def test_plan_default_order():
    want = [('block', 0, False), ('block', 1, False), ('block', 2, True)]
    for i in (3, 4, 5, 6):
        want += [('conv2', i, False), ('chain', i)]
    for i in range(7, 13):
        want += [('conv1', i)] * (i > 7) + [('conv2', i, False), ('conv3', i)]
    assert r50_steps(R()) == want


@pytest.mark.parametrize('blocks', [(3, 4, 6), (1, 1, 1), (2, 1), (1, 3)])
@pytest.mark.parametrize('route', list(TABLE))
def test_every_convolution_is_produced_once_and_in_order(route, blocks):
    """conv1, conv2 and conv3 + shortcut of every block: one producer each, conv1 before conv2 before conv3, block after block."""
    made = []
    for step in r50_steps(TABLE[route][0], blocks):
        kind, i = step[0], step[1]
        if kind == 'block':
            made += [(i, 1), (i, 2), (i, 3)] + ([(i + 1, 1)] if step[2] else [])
        elif kind == 'chain':
            made += [(i, 3), (i + 1, 1)]
        else:
            made.append((i, int(kind[-1])))
    assert made == [(i, c) for i in range(sum(blocks)) for c in (1, 2, 3)]


# ---- the launch list, with recorders in place of the ops.* constructors ----

class _Rec:
    def __init__(self, name, a, kw):
        self.name, self.a, self.kw = name, a, kw


class _Pack(dict):
    """One tagged tensor per key; projection shortcuts (c3ds) on the first block of every layer, as pack.py makes them."""

    def __contains__(self, k):
        return k != 'pe.w' and (not k.endswith('.c3ds.w') or k.split('.')[2] == '0')

    def __missing__(self, k):
        self[k] = torch.empty(0, dtype=torch.float32 if k.endswith('.b') else torch.bfloat16)
        return self[k]


OPS = {'conv2d': 'rmem_conv2d_nhwc', 'conv1x1_dual': 'rmem_conv1x1_dual_nhwc', 'bneck_chain': 'rmem_bneck_chain', 'bneck_block64': 'rmem_bneck_block64',
       'conv3x3_direct': 'rmem_conv3x3_direct', 'stem7x7s2': 'rmem_stem7x7s2', 'stem7x7s2_pool': 'rmem_stem7x7s2_pool',
       'maxpool3x3s2': 'rmem_maxpool3x3s2_nhwc', 'image_ptrs_to_nhwc4p': 'rmem_image_ptrs_to_nhwc4p', 'image_ptrs_to_nhwc8': 'rmem_image_ptrs_to_nhwc8'}


@pytest.fixture
def encoder(monkeypatch):
    """BatchEncoder on the CPU at 2 images of 97 x 129 whose prog() is a list of recorded calls (name, operands, keywords)."""
    from rmem_ocu_amd import encoder_batch, ops
    for fn, name in OPS.items():
        monkeypatch.setattr(ops, fn, lambda *a, _n=name, **kw: _Rec(_n, a, kw))
    monkeypatch.setattr(ops, 'PinnedRing', lambda *a: None)
    monkeypatch.setattr(ops, 'stem_padded_size', lambda H, W: (H + 10, W + 12))
    return lambda routes, B=2: encoder_batch.BatchEncoder(_Pack(), (97, 129), B, 'cpu', routes=routes)


@pytest.mark.parametrize('route', list(TABLE))
def test_launch_names_per_route(encoder, route):
    routes, launches, nblock, nchain, ndirect, ndual, nconv = TABLE[route]
    enc = encoder(routes)
    names = [o.name for o in enc.prog()]
    assert enc.prog() is enc.prog()
    assert len(names) == launches
    got = tuple(names.count(n) for n in ('rmem_bneck_block64', 'rmem_bneck_chain', 'rmem_conv3x3_direct', 'rmem_conv1x1_dual_nhwc', 'rmem_conv2d_nhwc'))
    assert got == (nblock, nchain, ndirect, ndual, nconv)
    assert enc.routes.front_split == (2 if routes.front_split == 2 else 1)
    assert (enc.mid_a128 is not None) == (enc.routes.front_split > 1)


def test_launch_order_default(encoder):
    names = [o.name for o in encoder(R()).prog()]
    assert names == (['rmem_image_ptrs_to_nhwc4p', 'rmem_stem7x7s2_pool'] + ['rmem_bneck_block64'] * 3 + ['rmem_conv2d_nhwc', 'rmem_bneck_chain'] * 4
                     + ['rmem_conv2d_nhwc', 'rmem_conv1x1_dual_nhwc'] + ['rmem_conv2d_nhwc'] * 15)


def test_encoder_resolves_what_depends_on_its_arguments(encoder, monkeypatch):
    assert encoder(R(block1=True, chain=(2,))).routes == R(block1=False, chain=(2,))          # block1 needs layer 1 chained
    assert encoder(R(front_split=0)).routes.front_split == 1 and encoder(R(front_split=-1)).routes.front_split == 1
    assert encoder(R(front_split=4), B=8).routes.front_split == 4 and encoder(R(front_split=3), B=8).routes.front_split == 1
    monkeypatch.setattr(_Pack, '__contains__', lambda self, k: k not in ('pe.w', 'stem.w4'))
    enc = encoder(R())                                                                         # a pack without stem.w4
    assert enc.routes.stem == 'rowrun' and [o.name for o in enc.prog()][:3] == ['rmem_image_ptrs_to_nhwc8', 'rmem_conv2d_nhwc', 'rmem_maxpool3x3s2_nhwc']
    monkeypatch.setenv('RMEM_NO_BNECK_BLOCK', '1')                                             # routes=None: the environment, at construction
    enc = encoder(None)
    monkeypatch.delenv('RMEM_NO_BNECK_BLOCK')
    assert enc.routes.block1 is False and 'rmem_bneck_block64' not in [o.name for o in enc.prog()]


def _region(t):
    return t.untyped_storage().data_ptr(), t.storage_offset(), t.storage_offset() + t.numel()


def _maps_of(op):
    """(reads, writes) of a recorded launch as operand tensors, each with the map it is to the step that made the launch:
    ('a' | 'b' | 'y', d) conv1's, conv2's and the block's output of the block d after the step's own (block 0 reads the pooled stem
    output as the y of a block -1).  None: rmem_conv2d_nhwc and the stem's first launches, which do not say."""
    a, kw, n = op.a, op.kw, op.name
    if n in ('rmem_stem7x7s2_pool', 'rmem_maxpool3x3s2_nhwc'):
        return [], [(a[3] if n == 'rmem_stem7x7s2_pool' else a[1], ('y', 0))]
    if n == 'rmem_bneck_block64':
        return [(a[0], ('y', -1))], [(a[7], ('y', 0))] + ([(kw['a_next'], ('a', 1))] if 'a_next' in kw else [])
    if n == 'rmem_bneck_chain':
        return [(a[0], ('b', 0)), (kw.get('residual', kw.get('x2')), ('y', -1))], [(a[3], ('y', 0)), (a[6], ('a', 1))]
    if n == 'rmem_conv1x1_dual_nhwc':
        return [(a[0], ('b', 0)), (a[1], ('y', -1))], [(a[4], ('y', 0))]
    if n == 'rmem_conv3x3_direct':
        return [(a[0], ('a', 0))], [(a[3], ('b', 0))]
    return None


def _check_dataflow(enc):
    """Replay the launch list over interval maps of the buffers: every element a launch reads was last written by a launch that wrote
    the map the reader means (conv1's output of ITS block, ...), whichever sub-batch ran in between."""
    steps = r50_steps(enc.routes)
    nfront = sum(1 for s in steps if s[1] < N1)
    nstem = STEM_LAUNCHES[enc.routes.stem]
    sched = []
    for _ in range(enc.routes.front_split):
        sched += [None] * nstem + steps[:nfront]
    sched += steps[nfront:]
    prog = enc.prog()
    assert len(prog) == len(sched)
    owner = {}                                             # storage -> disjoint [(begin, end, map)]

    def write(t, tag):
        s, b, e = _region(t)
        cut = []
        for (b1, e1, t1) in owner.get(s, []):
            cut += [(b1, min(e1, b), t1)] * (b1 < b) + [(max(b1, e), e1, t1)] * (e1 > e)
        owner[s] = sorted([c for c in cut if c[0] < c[1]] + [(b, e, tag)])

    def read(t, tag, what):
        s, b, e = _region(t)
        hit = [(max(b1, b), min(e1, e), t1) for (b1, e1, t1) in owner.get(s, []) if b1 < e and e1 > b]
        assert sum(e1 - b1 for b1, e1, _ in hit) == e - b, f'{what}: reads {tag} where nothing was written'
        wrong = sorted({t1 for _, _, t1 in hit if t1 != tag})
        assert not wrong, f'{what}: reads {tag}, finds {wrong}'

    for k, (op, step) in enumerate(zip(prog, sched)):
        m = _maps_of(op)
        if step is None:                                   # the stem: the launch that writes the pooled map is block -1
            if m is None:
                continue
            step = ('stem', -1)
        kind, i = step[0], step[1]
        if m is None:                                    # rmem_conv2d_nhwc: which convolution it is comes from the step
            src, dst = {'conv1': (('y', -1), ('a', 0)), 'conv2': (('a', 0), ('b', 0)), 'conv3': (('b', 0), ('y', 0))}[kind]
            m = [(op.a[0], src)] + ([(op.kw['residual'], ('y', -1))] if kind == 'conv3' else []), [(op.a[3], dst)]
        for t, (c, d) in m[0]:
            read(t, (c, i + d), f'launch {k} {op.name} {step}')
        for t, (c, d) in m[1]:
            write(t, (c, i + d))
    return owner


@pytest.mark.parametrize('B', [2, 4])
@pytest.mark.parametrize('route', list(TABLE))
def test_every_map_is_read_from_its_producer(encoder, route, B):
    """In particular with the front split: no launch of one sub-batch writes a region of mid_a that a later launch reads for another
    map (layer 2's first conv1 output, written per sub-batch while layer 1 still runs, has its own buffer for that)."""
    enc = encoder(TABLE[route][0], B=B)
    owner = _check_dataflow(enc)
    for t, tag in zip(enc.enc_out, (('y', 2), ('y', 6), ('y', 12))):          # the stage outputs hold the last block of every layer
        s, b, e = _region(t)
        assert {t1 for _, _, t1 in owner[s]} == {tag} and sum(e1 - b1 for b1, e1, _ in owner[s]) == e - b


def test_the_dataflow_check_sees_the_mid_a_overlap(encoder):
    """The check of the check: with layer 2's first conv1 output put back into mid_a, a split front overwrites it."""
    enc = encoder(R(front_split=2, block1=False))
    blk = enc.blocks[N1]
    assert blk.a.untyped_storage().data_ptr() == enc.mid_a128.untyped_storage().data_ptr()
    assert all(r.a.untyped_storage().data_ptr() == enc.mid_a.untyped_storage().data_ptr() for r in enc.blocks if r is not blk)
    blk.a = enc.mid_a[:blk.a.numel()].view(blk.a.shape)
    with pytest.raises(AssertionError, match=r"reads \('a', 3\), finds"):
        _check_dataflow(enc)
