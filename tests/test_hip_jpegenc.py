"""Baseline-JPEG output on the MI355X (rmem_jpeg_encode_rgb8, rmem_overlay_rgb8, rmem_ocu_amd.jpeg, evaluator.save_overlays).  The
yardstick is exact bytes: every device file equals the numpy restatement's file (tests/jpegenc_ref.py), whose entropy-coded segment
tests/test_jpegenc_host.py pins to Pillow's byte for byte."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegenc_ref as E
from boundary_ref import blobs

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def reference(name, restart_rows):
    rgb, quality = E.case(name)
    return E.file_bytes(rgb, quality, restart_rows)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                            # a copy: the cases are read-only


def device_files(rgb, labels=None, **kw):
    """rgb / labels: numpy or device tensors -> (list of the n files, offsets as a list)"""
    from rmem_ocu_amd import jpeg
    t = rgb if isinstance(rgb, torch.Tensor) else dev(rgb)
    lab = labels if labels is None or isinstance(labels, torch.Tensor) else dev(labels)
    out, offsets = jpeg.encode_files(t, lab, **kw)
    assert out.dtype == torch.uint8 and offsets.dtype == torch.int64 and out.is_cuda and offsets.is_cuda
    n = 1 if t.dim() == 3 else t.shape[0]
    assert offsets.shape == (n + 1,)
    off = offsets.cpu().tolist()
    data = out.cpu().numpy().tobytes()
    return [data[off[i]:off[i + 1]] for i in range(n)], off


def same(got, want, what=''):
    first = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), None)
    assert got == want, f'{what}: first differing byte {first} of {len(want)} (got {len(got)} bytes)'


@pytest.mark.parametrize('restart_rows', (0, 1))
@pytest.mark.parametrize('name', E.case_names())
def test_file_equals_restatement(name, restart_rows):
    from rmem_ocu_amd import _lib
    rgb, quality = E.case(name)
    want = reference(name, restart_rows)
    got, off = device_files(rgb, quality=quality, restart_rows=restart_rows)
    assert off == [0, len(want)]
    same(got[0], want, name)
    assert len(got[0]) <= _lib.lib().rmem_jpeg_encode_bound(rgb.shape[0], rgb.shape[1])


def three_frames():
    H, W = 40, 50
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([128 + 100 * np.sin(xx / 6.0 + c) * np.cos(yy / 4.0) for c in range(3)], -1).astype(np.uint8)
    smooth[blobs(H, W, 5, seed=8) > 0] //= 2
    return np.stack([np.full((H, W, 3), 77, np.uint8), smooth, rs.randint(0, 256, (H, W, 3)).astype(np.uint8)])


def test_stack_of_different_frames():
    frames = three_frames()
    want = [E.file_bytes(f, 90, 1) for f in frames]
    got, off = device_files(frames)
    assert off == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
    assert len(got[0]) < len(got[1]) < len(got[2])
    for i in range(3):
        same(got[i], want[i], f'frame {i}')
        same(device_files(frames[i])[0][0], got[i], f'frame {i} alone')     # a frame's file does not depend on its neighbours


def test_65_frames_cross_the_chunk():
    from rmem_ocu_amd import jpeg
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (65, 24, 40, 3)).astype(np.uint8)
    frames[::3] //= 8
    assert jpeg.CHUNK == 64
    files = jpeg.encode_rgb_stack(dev(frames), quality=80)
    assert len(files) == 65
    for i in range(65):
        same(files[i], E.file_bytes(frames[i], 80, 1), f'frame {i}')


def test_257_frames_cross_the_offsets_scan_step():
    """the frame-offsets scan carries its total over a 256-frame step: three frames of different file sizes, cycled"""
    kinds = [E._smooth(np.random.RandomState(s), 16, 16) for s in (1, 2, 3)]
    want = [E.file_bytes(k, 90, 1) for k in kinds]
    assert len({len(w) for w in want}) == 3
    got, off = device_files(np.stack([kinds[i % 3] for i in range(257)]), quality=90, restart_rows=1)
    assert off == np.concatenate(([0], np.cumsum([len(want[i % 3]) for i in range(257)]))).tolist()
    for i in range(257):
        same(got[i], want[i % 3], f'frame {i}')


def test_257_intervals_cross_the_interval_scan_step():
    """257 MCU rows, one restart interval each: the scan of the interval sizes carries over a 256-interval step"""
    from rmem_ocu_amd import _lib
    rgb = E._smooth(np.random.RandomState(1), 4112, 16)
    want = E.file_bytes(rgb, 90, 1)
    assert len(want) == 42295 and sum(want[i] == 0xFF and 0xD0 <= want[i + 1] <= 0xD7 for i in range(len(want) - 1)) == 256
    got, off = device_files(rgb, quality=90, restart_rows=1)
    assert off == [0, len(want)]
    same(got[0], want, '4112x16')
    assert len(got[0]) <= _lib.lib().rmem_jpeg_encode_bound(4112, 16)


def test_round_trip_through_the_device_decoder():
    from rmem_ocu_amd import jpeg
    for name in ('odd_37x53', 'tall_150x35', 'noise_q100_64x50'):
        for rr in (0, 1):
            rgb, quality = E.case(name)
            files, _ = device_files(rgb, quality=quality, restart_rows=rr)
            back = jpeg.decode(files, DEV).cpu().numpy()
            assert np.array_equal(back[0], np.array(Image.open(io.BytesIO(files[0])))), (name, rr)


def overlay_inputs(H, W, seed):
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    lab = np.stack([blobs(H, W, 5, seed=seed), blobs(H, W, 4, seed=seed + 1)])
    lab[1][lab[1] == 3] = 255
    lab[0, :3, :5] = 255                                                    # a label on the image border
    return rgb, lab


@pytest.mark.parametrize('alpha', (0.4, 1.0))
@pytest.mark.parametrize('size', ((37, 53), (16, 1300)))
def test_overlay_equals_reference(size, alpha):
    from rmem_ocu_amd import jpeg
    rgb, lab = overlay_inputs(*size, seed=11)
    assert 255 in lab and len(np.unique(lab)) >= 5
    got = jpeg.overlay(dev(rgb), dev(lab), alpha=alpha).cpu().numpy()
    want = np.stack([E.overlay(r, l, int(round(256 * alpha))) for r, l in zip(rgb, lab)])
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:4]
    grey = [v for i in range(256) for v in (i, 255 - i, 7)]
    got = jpeg.overlay(dev(rgb[0]), dev(lab[0]), alpha=alpha, palette=grey).cpu().numpy()
    assert np.array_equal(got[0], E.overlay(rgb[0], lab[0], int(round(256 * alpha)), grey))


@pytest.mark.parametrize('size', ((37, 53), (16, 1300)))
def test_fused_overlay_equals_overlay_then_encode(size):
    from rmem_ocu_amd import jpeg
    rgb, lab = overlay_inputs(*size, seed=21)
    fused, _ = device_files(rgb, lab, quality=85)
    split, _ = device_files(jpeg.overlay(dev(rgb), dev(lab)), quality=85)
    for i in range(2):
        same(fused[i], split[i], f'frame {i}')
        same(fused[i], E.file_bytes(E.overlay(rgb[i], lab[i], 102), 85, 1), f'frame {i} against the restatement')
    plain, _ = device_files(rgb, quality=85)
    assert plain[0] != fused[0]


def test_save_overlays(tmp_path):
    from rmem_ocu_amd import evaluator
    from rmem_ocu_amd._lib import RmemError
    rgb, lab = overlay_inputs(37, 53, seed=31)
    paths = [str(tmp_path / f'{i:05d}.jpg') for i in range(2)]
    evaluator.save_overlays(dev(rgb), dev(lab), paths, quality=80, alpha=0.5)
    for i, p in enumerate(paths):
        im = Image.open(p)
        im.load()
        assert im.size == (53, 37) and im.mode == 'RGB'
        same(open(p, 'rb').read(), E.file_bytes(E.overlay(rgb[i], lab[i], 128), 80, 1), p)
    with pytest.raises(RmemError, match='paths'):
        evaluator.save_overlays(dev(rgb), dev(lab), ['only_one.jpg'])


def test_bad_inputs_raise_with_a_message():
    from rmem_ocu_amd import jpeg
    from rmem_ocu_amd._lib import RmemError
    rgb = torch.zeros(2, 40, 50, 3, dtype=torch.uint8, device=DEV)
    lab = torch.zeros(2, 40, 50, dtype=torch.uint8, device=DEV)
    for fn in (jpeg.encode_files, jpeg.encode_rgb_stack):
        with pytest.raises(RmemError, match='device'):
            fn(rgb.cpu())
        with pytest.raises(RmemError, match='device'):
            fn(rgb, lab.cpu())
        with pytest.raises(RmemError, match='uint8'):
            fn(rgb.float())
        with pytest.raises(RmemError, match='uint8'):
            fn(rgb, lab.int())
        with pytest.raises(RmemError, match='non-empty'):
            fn(rgb[:0])
        with pytest.raises(RmemError, match='non-empty'):
            fn(rgb[..., :2])
        with pytest.raises(RmemError, match='matching'):
            fn(rgb, lab[:1])
        with pytest.raises(RmemError, match='matching'):
            fn(rgb, lab[:, :, :49])
        with pytest.raises(RmemError, match='quality'):
            fn(rgb, quality=0)
        with pytest.raises(RmemError, match='alpha'):
            fn(rgb, lab, alpha=1.5)
        with pytest.raises(RmemError, match='palette'):
            fn(rgb, lab, palette=[0, 0, 0])
    with pytest.raises(RmemError, match='device'):
        jpeg.overlay(rgb, lab.cpu())
    with pytest.raises(RmemError, match='labels'):
        jpeg.overlay(rgb, None)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RmemError, match='labels on'):
            jpeg.encode_files(rgb, lab.to('cuda:1'))


def test_two_streams_at_once():
    from rmem_ocu_amd import _codec, jpeg, png
    frames = three_frames()
    rgb_b, lab_b = overlay_inputs(37, 53, seed=41)
    want_a, off_a = device_files(frames)
    want_b, off_b = device_files(rgb_b, lab_b)
    ta, tb, tl = dev(frames), dev(rgb_b), dev(lab_b)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    with torch.cuda.stream(sa):
        out_a, offs_a = jpeg.encode_files(ta)
    with torch.cuda.stream(sb):
        out_b, offs_b = jpeg.encode_files(tb, tl)
    with torch.cuda.stream(sa):
        out_a2, offs_a2 = jpeg.encode_files(ta)
    sa.synchronize()
    sb.synchronize()
    ws, ka, kb = _codec._workspaces, ('jpeg.encode', DEV.index, sa.cuda_stream), ('jpeg.encode', DEV.index, sb.cuda_stream)
    assert ka in ws and kb in ws
    assert ws[ka].data_ptr() != ws[kb].data_ptr()
    for out, offs, want, off in ((out_a, offs_a, want_a, off_a), (out_b, offs_b, want_b, off_b), (out_a2, offs_a2, want_a, off_a)):
        o = offs.cpu().tolist()
        data = out.cpu().numpy().tobytes()
        assert o == off and [data[o[i]:o[i + 1]] for i in range(len(want))] == want
    before = ws[ka]
    with torch.cuda.stream(sa):
        jpeg.encode_files(ta[:1])                                           # a smaller call keeps the workspace
        png.encode_zlib(tl)                                                 # another codec on the same stream: a buffer of its own
    sa.synchronize()
    assert ws[ka] is before
    assert ws[('png.encode', DEV.index, sa.cuda_stream)].data_ptr() != ws[ka].data_ptr()
