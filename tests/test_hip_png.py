"""Palette-PNG output on the MI355X (rmem_png_encode_labels, rmem_ocu_amd.png, evaluator.save_masks).  Every case asserts two
things: (a) the device's zlib stream equals the Python restatement's bytes (tests/png_ref.py) exactly, and the offsets are the
running sums of the stream sizes; (b) the wrapped file decodes in Pillow to the input: pixels, mode and palette."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as P
from boundary_ref import blobs

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def reference(name):
    return P.zlib_stream(P.case(name))


def device_streams(labels, lut=None):
    """labels: numpy [n, H, W] or [H, W], or a device tensor -> (list of the n zlib streams, offsets as a list)"""
    from rmem_ocu_amd import png
    t = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels)).to(DEV)
    out, offsets = png.encode_zlib(t, None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.uint8)).to(DEV))
    assert out.dtype == torch.uint8 and offsets.dtype == torch.int64 and out.is_cuda and offsets.is_cuda
    n = 1 if t.dim() == 2 else t.shape[0]
    assert offsets.shape == (n + 1,)
    off = offsets.cpu().tolist()
    data = out.cpu().numpy().tobytes()
    return [data[off[i]:off[i + 1]] for i in range(n)], off


def decodes_to(data, lab):
    from rmem_ocu_amd.evaluator import _davis_palette
    im = Image.open(io.BytesIO(data))
    im.load()
    return im.mode == 'P' and im.size == (lab.shape[1], lab.shape[0]) and np.array_equal(np.array(im), lab) and im.getpalette() == _davis_palette()


def check_stack(labels, refs=None, lut=None):
    """(a) and (b) for a numpy stack [n, H, W]"""
    from rmem_ocu_amd import png
    labels = np.asarray(labels, dtype=np.uint8)
    refs = refs or [P.zlib_stream(lab, lut) for lab in labels]
    got, off = device_streams(labels, lut)
    assert off == np.concatenate(([0], np.cumsum([len(r) for r in refs]))).tolist()
    for i, (g, r) in enumerate(zip(got, refs)):
        assert g == r, f'frame {i}: first differing byte {next((k for k in range(min(len(g), len(r))) if g[k] != r[k]), None)} of {len(r)}'
        want = labels[i] if lut is None else np.asarray(lut, dtype=np.uint8)[labels[i]]
        assert decodes_to(png.wrap(g, *labels[i].shape), want)
    return got


@pytest.mark.parametrize('name', P.case_names())
def test_stream_equals_restatement(name):
    lab = P.case(name)
    got = check_stack(lab[None], [reference(name)])
    assert len(got[0]) <= P.zlib_bound(*lab.shape)


def three_frames():
    H, W = 40, 50
    return np.stack([np.zeros((H, W), np.uint8), blobs(H, W, 5, seed=8), np.random.RandomState(5).randint(0, 256, (H, W)).astype(np.uint8)])


def test_stack_of_different_frames():
    labels = three_frames()
    got = check_stack(labels)
    assert len(got[0]) < len(got[1]) < len(got[2])
    for i in range(3):                                 # a frame's stream does not depend on its neighbours in the stack
        assert device_streams(labels[i])[0][0] == got[i]


def test_65_frames_cross_the_chunk():
    from rmem_ocu_amd import png
    rs = np.random.RandomState(3)
    labels = np.stack([blobs(8, 9, 4, seed=100 + i) if i % 3 else rs.randint(0, 256, (8, 9)).astype(np.uint8) for i in range(65)])
    assert png.CHUNK == 64
    files = png.encode_label_stack(torch.from_numpy(labels).to(DEV))
    assert len(files) == 65
    for i in range(65):
        assert files[i] == P.png_file(labels[i]), i
        assert decodes_to(files[i], labels[i])


def test_257_frames_cross_the_offsets_scan_step():
    """the frame-offsets scan carries its total over a 256-frame step: three maps of different stream sizes, cycled, one call"""
    from rmem_ocu_amd import png
    kinds = [np.zeros((4, 70), np.uint8), blobs(4, 70, 3, seed=1), np.random.RandomState(2).randint(0, 256, (4, 70)).astype(np.uint8)]
    want = [P.zlib_stream(k) for k in kinds]
    assert len({len(w) for w in want}) == 3
    got, off = device_streams(np.stack([kinds[i % 3] for i in range(257)]))
    assert off == np.concatenate(([0], np.cumsum([len(want[i % 3]) for i in range(257)]))).tolist()
    for i in range(257):
        assert got[i] == want[i % 3], i
    for i in range(3):
        assert decodes_to(png.wrap(got[254 + i], 4, 70), kinds[(254 + i) % 3])


def test_non_contiguous_view():
    labels = np.stack([blobs(40, 50, 5, seed=40 + i) for i in range(3)])
    view = torch.from_numpy(labels).to(DEV)[:, ::2]
    assert not view.is_contiguous()
    got, _ = device_streams(view)
    assert got == [P.zlib_stream(lab[::2]) for lab in labels]


def test_stale_state_does_not_leak():
    """noise, then an empty map, into the same out / workspace on the same stream (the C entry point, buffers held here)"""
    from rmem_ocu_amd import _lib
    H, W = 64, 200
    noise = torch.from_numpy(P.case('noise9_64x200')).to(DEV)
    empty = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    L = _lib.lib()
    ws = torch.empty(L.rmem_png_workspace_bytes(1, H, W), dtype=torch.uint8, device=DEV)
    out = torch.empty(L.rmem_png_zlib_bound(H, W), dtype=torch.uint8, device=DEV)
    offsets = torch.empty(2, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    results = []
    for lab in (noise, empty):
        _lib.check(L.rmem_png_encode_labels(lab.data_ptr(), 1, H, W, None, ws.data_ptr(), out.data_ptr(), offsets.data_ptr(), stream),
                   'rmem_png_encode_labels')
        off = offsets.cpu().tolist()
        results.append(out.cpu().numpy().tobytes()[off[0]:off[1]])
    assert results[0] == reference('noise9_64x200')
    fresh, _ = device_streams(np.zeros((H, W), np.uint8))
    assert results[1] == fresh[0] == P.zlib_stream(np.zeros((H, W), np.uint8))


def test_lut():
    from rmem_ocu_amd import png
    lab = blobs(33, 70, 3, seed=6)
    assert set(np.unique(lab).tolist()) == {0, 1, 2}
    lut = P.squeeze_lut([0, 4, 9])
    check_stack(lab[None], lut=lut)
    files = png.encode_label_stack(torch.from_numpy(lab).to(DEV), squeeze_idx=[0, 4, 9])
    assert files[0] == P.png_file(lab, lut)
    decoded = np.array(Image.open(io.BytesIO(files[0])))
    assert set(np.unique(decoded).tolist()) == {0, 4, 9} and np.array_equal(decoded, lut[lab])
    plain = png.encode_label_stack(torch.from_numpy(lab).to(DEV))
    assert np.array_equal(np.array(Image.open(io.BytesIO(plain[0]))), lab)


def test_non_default_stream():
    labels = three_frames()
    want, want_off = device_streams(labels)
    t = torch.from_numpy(labels).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    from rmem_ocu_amd import png
    with torch.cuda.stream(side):
        out, offsets = png.encode_zlib(t)
    side.synchronize()
    off = offsets.cpu().tolist()
    data = out.cpu().numpy().tobytes()
    assert off == want_off and [data[off[i]:off[i + 1]] for i in range(3)] == want


def test_bad_inputs_raise_with_a_message():
    from rmem_ocu_amd import png
    from rmem_ocu_amd._lib import RmemError
    a = torch.zeros(2, 40, 50, dtype=torch.uint8, device=DEV)
    with pytest.raises(RmemError, match='uint8'):
        png.encode_zlib(a.float())
    with pytest.raises(RmemError, match='non-empty'):
        png.encode_zlib(a[:0])
    with pytest.raises(RmemError, match='non-empty'):
        png.encode_zlib(a[None])
    with pytest.raises(RmemError, match='lut'):
        png.encode_zlib(a, lut=torch.zeros(255, dtype=torch.uint8, device=DEV))


def test_group_slot_masks_to_png_files(synth_weights, tmp_path):
    """a GroupSlot run at the engine tests' small geometry: every clip's predicted masks through encode_label_stack and save_masks"""
    from rmem_ocu_amd import build_vos_model, evaluator, get_config, png
    from rmem_ocu_amd.clip_runner import GroupSlot
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from rmem_ocu_amd.synth import make_clip
    B, n = 2, 5
    clips = [make_clip(40 + c, n, 161, 193, 3) for c in range(B)]
    cfg = get_config('pre_vost', 'test', 'r50_aotl')
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 2
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_weights)
    ge = GroupEngine(model, B, 0, 5, lookahead=2)
    gs = GroupSlot(ge, (160, 192), DEV)
    gs.start([f.to(DEV) for f, _ in clips], [m.to(DEV) for _, m in clips], 3)
    while not gs.done:
        gs.step()
    ge.synchronize()
    for c in range(B):
        want = gs.labels[c, 1:n].cpu().numpy()
        assert want.max() > 0
        files = png.encode_label_stack(gs.labels[c, 1:n])
        assert len(files) == n - 1
        for i in range(n - 1):
            assert decodes_to(files[i], want[i])
        paths = [str(tmp_path / f'clip{c}_{i:05d}.png') for i in range(1, n)]
        evaluator.save_masks(gs.labels[c, 1:n], paths)
        for i, p in enumerate(paths):
            assert np.array_equal(np.array(Image.open(p)), want[i])
    with pytest.raises(evaluator._lib.RmemError, match='paths'):
        evaluator.save_masks(gs.labels[0, 1:n], ['only_one.png'])
