"""The geodesic nearest-site transform on the MI355X against tests/geodesic_ref.py: exact integer equality of whole arrays of all
three outputs, no tolerance.  Labels and image sit between guard bytes and start at any byte; outputs and workspace are dirtied
first and followed by guards.  The shapes are placed round the core tile (th, tw) of a round: one pixel, one row, one column, a
tile less one row and plus one column, whole tiles, and a frame of 3 x 3 tiles whose last ones are slivers.  The keys of a (shape,
image, labels, site set, weights) are computed once on the host (the Jacobi restatement; Dijkstra for the serpentine) and shared
by every limit, which is a threshold on them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geodesic_ref as R

pytestmark = pytest.mark.gpu

S = R.SENTINEL
CANARY = 0xA5
CANARY32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
OFFSETS = (0, 1, 3, 13)
WEIGHTS = ((1, 0), (1, 1), (64, 64), (5, 2))
FILLS = (None, (0,), (0, 255), (0, 1, 3))
ALL = (True, True, True)
MAX_CALLS = 400                                                      # of the raw loop: far above any case here


@functools.lru_cache(maxsize=None)
def _tile():
    from rmem_ocu_amd import distance
    return distance.geodesic_tile()


def _shapes():
    th, tw = _tile()
    return [(1, 1, 1), (1, 1, tw + 6), (1, th + 6, 1), (2, th - 1, tw + 1), (3, th, tw), (1, th + 1, 2 * tw + 1), (2, 2 * th + 33, 2 * tw + 3)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _image(kind, shape, C):
    a = R.make_image(kind, shape, C, _tile()[1])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _labels(kind, shape):
    a = R.make_labels(kind, shape)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _keys(shape, image, C, labels, sites, weights):
    k = R.jacobi(_labels(labels, shape), _image(image, shape, C), sites, *weights)
    k.setflags(write=False)
    return k


def _a_cost(keys):
    """a value equal to one pixel's cost in the reference: the median of the costs there are"""
    cost = keys >> R.SHIFT
    real = np.sort(cost[cost != S])
    return int(real[real.size // 2]) if real.size else 7


def _guarded(dev, a, offset):
    """a's bytes on the device between guard bytes, starting `offset` bytes past a 64-byte boundary -> (buffer, view, front)"""
    front = 64 + offset
    buf = torch.full((front + a.size + 64,), CANARY, dtype=torch.uint8)
    buf[front:front + a.size] = torch.from_numpy(a.copy()).reshape(-1)
    buf = buf.to(dev)
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + a.size], front


def _words(values):
    return None if values is None else (ctypes.c_uint * 8)(*R.bits(values))


def _run(dev, labels, image, sites, fill=None, weights=(1, 1), limits=(-1,), offset=0, outs=ALL, batch=8):
    """begin, rounds until no tile changed, finish on guarded copies, once per limit -> ([(index, cost, taken) per limit], [rounds
    per limit]); the outputs asked for and the workspace are dirtied and followed by guards"""
    from rmem_ocu_amd import _lib
    L = _lib.lib()
    n, H, W = labels.shape
    C = 1 if image.ndim == 3 else image.shape[-1]
    m, size = len(limits), labels.size
    stream = torch.cuda.current_stream(dev).cuda_stream
    lbuf, lview, lfront = _guarded(dev, labels, offset)
    ibuf, iview, ifront = _guarded(dev, image, OFFSETS[(OFFSETS.index(offset) + 1) % 4])
    need = int(L.rmem_label_geodesic_workspace_bytes(n, H, W))
    assert need % 16 == 0 and need >= 16 * size
    index, cost, ws = (torch.full((k + 64,), CANARY32, dtype=torch.int32, device=dev) for k in (m * size, m * size, need // 4))
    taken = torch.full((m * size + 64,), CANARY, dtype=torch.uint8, device=dev)
    changed = torch.full((n + 16,), CANARY32, dtype=torch.int32, device=dev)
    ran = []
    for k, limit in enumerate(limits):
        ws[:need // 4] = CANARY32                                    # prior contents of the workspace do not matter at begin
        _lib.check(L.rmem_label_geodesic_begin(lview.data_ptr(), n, H, W, _words(sites), ws.data_ptr(), need, stream), 'begin')
        rounds = 0
        for _ in range(MAX_CALLS):
            _lib.check(L.rmem_label_geodesic_rounds(iview.data_ptr(), C, n, H, W, weights[0], weights[1], limit, rounds, batch, changed.data_ptr(),
                                                    ws.data_ptr(), need, stream), 'rounds')
            rounds += batch
            c = changed.cpu().numpy()
            assert (c[n:] == CANARY32).all() and (c[:n] >= 0).all(), 'changed: n counters, nothing beyond'
            if not c[:n].any():
                break
        else:
            raise AssertionError('the rounds did not come to rest')
        ran.append(rounds)
        ptr = [t[k * size:].data_ptr() if want else None for t, want in zip((index, cost, taken), outs)]
        _lib.check(L.rmem_label_geodesic_finish(lview.data_ptr(), n, H, W, _words(fill), limit, rounds, ptr[0], ptr[1], ptr[2], ws.data_ptr(), need,
                                                stream), 'finish')
    torch.cuda.synchronize()
    for buf, front, a, what in ((lbuf, lfront, labels, 'labels'), (ibuf, ifront, image, 'image')):
        h = buf.cpu().numpy()
        assert (h[:front] == CANARY).all() and (h[front + a.size:] == CANARY).all(), 'guard bytes around the ' + what
        assert np.array_equal(h[front:front + a.size], a.reshape(-1)), 'the %s are read only' % what
    host = [index.cpu().numpy(), cost.cpu().numpy(), taken.cpu().numpy()]
    for t, want, canary in zip(host, outs, (CANARY32, CANARY32, CANARY)):
        assert (t[m * size if want else 0:] == canary).all(), 'beyond an output, or an output not asked for, was written'
    assert (ws[need // 4:] == CANARY32).all().item(), 'ints beyond the workspace were written'
    return [tuple(t[k * size:(k + 1) * size].reshape(labels.shape) if want else None for t, want in zip(host, outs)) for k in range(m)], ran


def _same(got, want):
    return all(g is None or np.array_equal(g, w) for g, w in zip(got, want))


def _where(got, want):
    return [np.argwhere(g != w)[:4].tolist() for g, w in zip(got, want) if g is not None]


@pytest.mark.parametrize('image', R.IMAGES)
@pytest.mark.parametrize('si', range(7))
def test_transform(dev, si, image):
    """grey and colour; every site set, each with one of the label stacks, weights, fill sets and byte offsets, which change from
    set to set; every limit; all three outputs"""
    shape = _shapes()[si]
    for C in (1, 3):
        for k, sites in enumerate(R.SITE_SETS):
            j = k + C + si
            labels, weights, fill, offset = R.LABELS[j % 3], WEIGHTS[j % 4], FILLS[(j + 1) % 4], OFFSETS[(j + 2) % 4]
            keys = _keys(shape, image, C, labels, sites, weights)
            limits = (-1, 0, _a_cost(keys), 2 ** 30)
            got, _ = _run(dev, _labels(labels, shape), _image(image, shape, C), sites, fill, weights, limits, offset)
            for limit, g in zip(limits, got):
                want = R.finish(_labels(labels, shape), keys, fill, limit)
                assert _same(g, want), (shape, image, C, labels, sites, weights, fill, limit, offset, _where(g, want))


def test_generators_are_what_they_claim():
    th, tw = _tile()
    shape = _shapes()[6]
    assert shape == (2, 2 * th + 33, 2 * tw + 3)
    for kind, x in (('step-1', tw - 1), ('step', tw), ('step+1', tw + 1)):
        im = _image(kind, shape, 1)
        assert (im[:, :, :x] == 40).all() and (im[:, :, x:] == 200).all()
    wall = _image('wall', shape, 3)
    assert (wall[:, :, shape[2] // 2, 0] == 255).sum() == 2 * (shape[1] - 1) and wall[0, shape[1] - 2, shape[2] // 2, 0] == 0
    assert shape[1] - 2 >= 2 * th and shape[2] // 2 >= tw            # the gap lies in the last row of tiles, the wall beyond the first column
    keys = _keys(shape, 'wall', 1, 'ends', (3,), (1, 1))
    index, cost, _ = R.finish(_labels('ends', shape), keys)
    assert cost[0, 0, shape[2] // 2 + 1] > 5 * (shape[2] // 2 + 1) and (index >= 0).all()
    lim = _a_cost(keys)
    index, cost, _ = R.finish(_labels('ends', shape), keys, None, lim)
    assert (cost == lim).any() and (index < 0).any() and (index >= 0).any()
    assert (R.finish(_labels('sparse', shape), _keys(shape, 'random', 3, 'sparse', (), (1, 1)))[0] == -1).all()


def test_serpentine(dev, monkeypatch):
    """the cheapest path crosses tile boundaries dozens of times: tiles that went idle are woken again, the host loop runs more
    than one call, and the cap on a tile's passes decides nothing; with the skip switch off the bytes are the same"""
    from rmem_ocu_amd import distance
    th, tw = _tile()
    shape = (1, 2 * th + 33, 2 * tw + 3)
    labels, image = R.serpentine(shape)
    want = R.finish(labels, R.dijkstra(labels, image, (3,), 1, 64))
    assert (want[0] == 0).all() and want[1].max() > 5 * shape[1] * (shape[2] // 8 - 1)       # through every corridor
    d, im = torch.from_numpy(labels).to(dev), torch.from_numpy(image).to(dev)
    info = {}
    index, cost = distance.geodesic_nearest(d, im, (3,), spatial=1, colour=64, batch=2, info=info)
    assert _same((index.cpu().numpy(), cost.cpu().numpy()), want), _where((index.cpu().numpy(), cost.cpu().numpy()), want)
    assert info['rounds'] > 2 and info['calls'] > 1 and info['rounds'] == 2 * info['calls']
    print('serpentine: rounds', info['rounds'])
    monkeypatch.setenv('RMEM_GEODESIC_SKIP', '0')
    off = {}
    index0, cost0 = distance.geodesic_nearest(d, im, (3,), spatial=1, colour=64, batch=2, info=off)
    assert torch.equal(index0, index) and torch.equal(cost0, cost) and off['rounds'] == info['rounds']
    monkeypatch.delenv('RMEM_GEODESIC_SKIP')
    got, ran = _run(dev, labels, image, (3,), None, (1, 64), (-1,), 3, batch=1)             # the raw loop, a round per call
    assert _same(got[0], want) and 2 < ran[0] <= info['rounds']


def test_round_bound(dev):
    """uniform image, one site at index 0, a round per call: cheapest paths are monotone, so the tile at (i, j) is final after
    round i + j + 1 and one more round reports no change.  More rounds mean that a tile does not reach its fixed point."""
    from rmem_ocu_amd import distance
    th, tw = _tile()
    for si in (3, 5, 6):
        n, H, W = shape = _shapes()[si]
        labels = np.zeros(shape, dtype=np.uint8)
        labels[:, 0, 0] = 3
        image = _image('uniform', shape, 3)
        info = {}
        index, cost = distance.geodesic_nearest(torch.from_numpy(labels).to(dev), torch.from_numpy(image.copy()).to(dev), (3,), 1, 1, batch=1,
                                                info=info)
        assert (index == 0).all().item() and np.array_equal(cost.cpu().numpy()[0], R.chamfer(H, W, 0, 0))
        tiles_y, tiles_x = -(-H // th), -(-W // tw)
        print('round bound:', shape, info['rounds'], 'of', tiles_x + tiles_y + 1)
        assert info['rounds'] <= tiles_x + tiles_y + 1, (shape, info)


def test_every_byte_offset(dev):
    shape = _shapes()[5]
    for image, C, labels, sites in (('random', 3, 'blobs', (1, 2, 3)), ('step', 1, 'sparse', (3,))):
        keys = _keys(shape, image, C, labels, sites, (1, 1))
        for offset in OFFSETS:
            limits = (-1, _a_cost(keys))
            got, _ = _run(dev, _labels(labels, shape), _image(image, shape, C), sites, (0,), (1, 1), limits, offset)
            for limit, g in zip(limits, got):
                assert _same(g, R.finish(_labels(labels, shape), keys, (0,), limit)), (image, offset, limit)


def test_every_combination_of_outputs(dev):
    """an output that is not asked for is not written, and those asked for do not depend on the others"""
    shape = _shapes()[3]
    for image, C, labels, sites, fill in (('random', 3, 'blobs', (1, 2, 3), (0,)), ('wall', 1, 'sparse', (255,), (0, 3)),
                                          ('uniform', 1, 'ends', (), None)):
        keys = _keys(shape, image, C, labels, sites, (5, 2))
        for mask in range(1, 8):
            outs = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
            limits = (-1, _a_cost(keys))
            got, _ = _run(dev, _labels(labels, shape), _image(image, shape, C), sites, fill, (5, 2), limits, OFFSETS[mask % 4], outs)
            for limit, g in zip(limits, got):
                assert [x is not None for x in g] == list(outs)
                assert _same(g, R.finish(_labels(labels, shape), keys, fill, limit)), (image, outs, limit)


def test_python_functions_side_stream_and_passes(dev):
    """through the package: [H, W] as one frame with [H, W] and [H, W, C] images, return_cost, out=, max_cost; a side stream, twice,
    byte-identical; a workspace that forces three passes over five frames gives the bytes of one pass"""
    from rmem_ocu_amd import distance
    from rmem_ocu_amd._lib import RmemError
    shape = _shapes()[3]
    a, im = _labels('blobs', shape), _image('random', shape, 3)
    keys = _keys(shape, 'random', 3, 'blobs', (1, 2, 3), (1, 1))
    d, di = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(im.copy()).to(dev)
    index, cost = distance.geodesic_nearest(d, di, [1, 2, 3])
    assert index.dtype == cost.dtype == torch.int32 and index.shape == cost.shape == d.shape
    assert _same((index.cpu().numpy(), cost.cpu().numpy()), R.finish(a, keys))
    lim = _a_cost(keys)
    index, none = distance.geodesic_nearest(d[1], di[1], {1, 2, 3}, max_cost=lim, return_cost=False)
    assert none is None and index.shape == shape[1:] and np.array_equal(index.cpu().numpy(), R.finish(a, keys, None, lim)[0][1])
    grey = _image('random', shape, 1)
    g = torch.from_numpy(grey.copy()).to(dev)
    kg = _keys(shape, 'random', 1, 'blobs', (1, 2, 3, 255), (5, 2))
    grown = distance.geodesic_grow(d, g, spatial=5, colour=2)                                  # fill (0,), sites: the rest
    assert grown.dtype == torch.uint8 and grown.shape == d.shape and np.array_equal(grown.cpu().numpy(), R.finish(a, kg, (0,))[2])
    assert torch.equal(distance.geodesic_grow(d[0], g[0], spatial=5, colour=2), grown[0])
    assert torch.equal(distance.geodesic_grow(d, g[..., None], spatial=5, colour=2), grown)   # [n, H, W, 1] is grey too
    out = torch.full(shape, CANARY, dtype=torch.uint8, device=dev)
    assert distance.geodesic_grow(d, g, spatial=5, colour=2, out=out) is out and torch.equal(out, grown)
    assert torch.equal(d.cpu(), torch.from_numpy(a.copy())) and torch.equal(di.cpu(), torch.from_numpy(im.copy()))
    with pytest.raises(RmemError, match='out must be a contiguous uint8 tensor'):
        distance.geodesic_grow(d, g, out=out[:1])
    with pytest.raises(RmemError, match='out must not be the labels'):
        distance.geodesic_grow(d, g, out=d)
    with pytest.raises(RmemError, match='image must have the labels\' shape'):
        distance.geodesic_grow(d, di[:, :, :-1])
    with pytest.raises(RmemError, match='image must be contiguous'):
        distance.geodesic_grow(d, di.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))
    with pytest.raises(RmemError, match='image must be on the labels\' device'):
        distance.geodesic_grow(d, di.cpu())
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs = [distance.geodesic_nearest(d, di, (1, 2, 3)) + (distance.geodesic_grow(d, di, sites=(1, 2, 3)),) for _ in range(2)]
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert _same([t.cpu().numpy() for t in runs[0]], R.finish(a, keys, (0,)))
    five = (5,) + shape[1:]
    a5, i5 = R.make_labels('sparse', five, 3), R.make_image('random', five, 3, _tile()[1], 3)
    d5, di5 = torch.from_numpy(a5).to(dev), torch.from_numpy(i5).to(dev)
    one, three = {}, {}
    whole = distance.geodesic_nearest(d5, di5, (1, 2, 3), info=one)
    per_frame = int(distance._lib.lib().rmem_label_geodesic_workspace_bytes(1, *shape[1:]))
    parts = distance.geodesic_nearest(d5, di5, (1, 2, 3), workspace_bytes=2 * per_frame + 8, info=three)
    assert len(one['passes']) == 1 and [p['frames'] for p in three['passes']] == [2, 2, 1]
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    assert _same([t.cpu().numpy() for t in whole], R.finish(a5, R.jacobi(a5, i5, (1, 2, 3))))
    with pytest.raises(RmemError, match='workspace_bytes must be an integer of at least one frame\'s need'):
        distance.geodesic_nearest(d5, di5, (1, 2, 3), workspace_bytes=per_frame - 1)


def test_against_chamfer_and_grow(dev):
    """colour = 0, one site: the cost is spatial times the chamfer by hand.  A uniform image, a single site: geodesic_grow is
    distance.grow (no order of two sites to differ in), and so is the taken stack where the sites are everything but the fill"""
    from rmem_ocu_amd import distance
    n, H, W = shape = _shapes()[5]
    labels = np.zeros(shape, dtype=np.uint8)
    labels[0, H - 3, 70] = 2
    d = torch.from_numpy(labels).to(dev)
    noise, flat = torch.from_numpy(_image('random', shape, 3).copy()).to(dev), torch.from_numpy(_image('uniform', shape, 3).copy()).to(dev)
    for sp in (1, 5, 64):
        index, cost = distance.geodesic_nearest(d, noise, (2,), spatial=sp, colour=0)
        assert (index == (H - 3) * W + 70).all().item() and np.array_equal(cost.cpu().numpy()[0], sp * R.chamfer(H, W, H - 3, 70))
    for colour in (0, 1, 64):
        assert torch.equal(distance.geodesic_grow(d, flat, colour=colour), distance.grow(d))
    assert torch.equal(distance.geodesic_nearest(d, flat, (2,))[0], distance.nearest(d, (2,))[0])
    full = np.array(_labels('blobs', shape))
    full[full == 0] = 7
    full[0, 5:9, 60:90] = 0                                          # a hole of fill in a frame of sites: no pixel outside it changes
    f = torch.from_numpy(full).to(dev)
    got = distance.geodesic_grow(f, flat)
    assert torch.equal(got[f != 0], f[f != 0]) and (got != 0).all().item()
    assert np.array_equal(got.cpu().numpy(), R.finish(full, R.jacobi(full, _image('uniform', shape, 3), set(range(1, 256))), (0,))[2])


def test_evaluator_wrappers(dev):
    from rmem_ocu_amd import distance
    from rmem_ocu_amd.evaluator import fill_void, fill_void_geodesic, labels_from_seeds, labels_from_seeds_geodesic, snap_masks
    H, W, E = 20, 40, 25
    image = np.full((2, H, W, 3), 40, dtype=np.uint8)
    image[:, :, E:] = 200                                            # a step edge between columns 24 and 25
    im = torch.from_numpy(image).to(dev)
    seeds = np.zeros((2, H, W), dtype=np.uint8)                      # frame 1 has no seed
    seeds[0, 10, 5], seeds[0, 10, 30] = 1, 2                         # a click on either side of the edge
    s = torch.from_numpy(seeds).to(dev)
    plain, geo = labels_from_seeds(s).cpu().numpy(), labels_from_seeds_geodesic(s, im).cpu().numpy()
    assert (plain[0, :, :18] == 1).all() and (plain[0, :, 18:] == 2).all()                   # the midpoint between the clicks
    assert (geo[0, :, :E] == 1).all() and (geo[0, :, E:] == 2).all()                         # the edge
    assert np.array_equal(geo, R.finish(seeds, R.jacobi(seeds, image, set(range(1, 256))), (0,))[2])
    assert np.array_equal(geo[1], seeds[1]) and np.array_equal(plain[1], seeds[1])           # a frame without seeds: as it is
    assert torch.equal(labels_from_seeds_geodesic(s[1], im[1]), s[1])
    seeds[0, 3, 35] = 9                                              # a negative seed: it claims its region, which is then background
    s = torch.from_numpy(seeds).to(dev)
    want = R.finish(seeds, R.jacobi(seeds, image, set(range(1, 256))), (0,))[2]
    neg = labels_from_seeds_geodesic(s, im, background=9).cpu().numpy()
    assert np.array_equal(neg, np.where(want == 9, 0, want)) and (neg[0] == 0).sum() == (want[0] == 9).sum() > 0 and (want[0] != 0).all()
    lim = labels_from_seeds_geodesic(s, im, spatial=5, colour=2, max_cost=100).cpu().numpy()
    assert np.array_equal(lim, R.finish(seeds, R.jacobi(seeds, image, set(range(1, 256)), 5, 2), (0,), 100)[2]) and (lim[0] == 0).any()
    rim = np.zeros((1, H, W), dtype=np.uint8)                        # a 255 rim of five columns straddling the edge
    rim[:, :, :23], rim[:, :, 23:28] = 1, 255
    r = torch.from_numpy(rim).to(dev)
    mid, snapped = fill_void(r).cpu().numpy(), fill_void_geodesic(r, im[:1]).cpu().numpy()
    assert (mid[0, :, :26] == 1).all() and (mid[0, :, 26:] == 0).all()                       # the rim's middle (the tie to the first site)
    assert (snapped[0, :, :E] == 1).all() and (snapped[0, :, E:] == 0).all()                 # the edge
    assert np.array_equal(fill_void_geodesic(r, im[:1], void=1).cpu().numpy(), R.finish(rim, R.jacobi(rim, image[:1], (0, 255)), (1,))[2])
    moved = np.zeros((1, H, W), dtype=np.uint8)                      # a mask two pixels beyond the edge
    moved[:, :, :E + 2] = 1
    m = torch.from_numpy(moved).to(dev)
    back = snap_masks(m, im[:1], 3, keep_thin=False).cpu().numpy()
    assert (back[0, :, :E] == 1).all() and (back[0, :, E:] == 0).all()                       # returns to the edge
    kept = snap_masks(m, im[:1], 3).cpu().numpy()                    # keep_thin: against the band cut out here from the parts
    from rmem_ocu_amd import skeleton
    near = (distance.label_edt(m, border=False) <= 9) & (skeleton.thin(m) == 0)
    cut = np.where(near.cpu().numpy(), 255, moved).astype(np.uint8)
    assert (cut == 255).any() and np.array_equal(kept, R.finish(cut, R.jacobi(cut, image[:1], (0, 1)), (255,))[2])
    assert snap_masks(m[0], im[0], 3, keep_thin=False).shape == (H, W)
    line = np.zeros((1, H, W), dtype=np.uint8)                       # a one-pixel-wide object, thinner than the band
    line[0, 3:17, 10] = 2
    ln, flat = torch.from_numpy(line).to(dev), torch.full((1, H, W), 90, dtype=torch.uint8, device=dev)
    assert (snap_masks(ln, flat, 3, keep_thin=False) == 0).all().item()                      # it vanishes
    alive = snap_masks(ln, flat, 3).cpu().numpy()
    assert (alive[line == 2] == 2).all() and set(np.unique(alive)) == {0, 2}                 # with its skeleton kept it survives
