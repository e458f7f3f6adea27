"""Palette-PNG input on the MI355X (rmem_png_decode_labels, rmem_ocu_amd.png, evaluator.labels_from_pngs).  Every case of
tests/pnginf_ref.py's table must decode to exactly the label map it was built from -- which the CPU tier shows to be what Pillow and
this file's own inflate / unfilter / unpack give -- with a zero status word; damaged streams must end in their one status bit, a
zero-filled frame, and untouched memory around the buffers."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import pnginf_ref as R
import png_ref as P
from boundary_ref import blobs, shifted_speckled

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CANARY = 64


def expected(name):
    c = R.cases()[name]
    return c.label if c.lut is None else c.lut[c.label]


def raw_decode(files, lut=None, out_fill=0xA5, ws_fill=0xFF):
    """the C entry point with buffers held here: out and the workspace pre-filled, 64 canary bytes behind each ->
    (labels [n, H, W] numpy, status list, canaries intact)"""
    from rmem_ocu_amd import _lib, png
    pk = png.PackedPngs(files)
    n, H, W = pk.shape
    L = _lib.lib()
    nws = L.rmem_png_decode_workspace_bytes(n, H, W)
    ws = torch.full((nws + CANARY,), ws_fill, dtype=torch.uint8, device=DEV)
    out = torch.full((n * H * W + CANARY,), out_fill, dtype=torch.uint8, device=DEV)
    ws[nws:] = 0x5A
    out[n * H * W:] = 0x5A
    status = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    bits, descs = pk.buf.to(DEV), pk.desc_bytes.to(DEV)
    lut_d = None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.uint8)).to(DEV)
    _lib.check(L.rmem_png_decode_labels(bits.data_ptr(), descs.data_ptr(), n, H, W, None if lut_d is None else lut_d.data_ptr(),
                                        ws.data_ptr(), out.data_ptr(), status.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream),
               'rmem_png_decode_labels')
    torch.cuda.synchronize()
    intact = bool((ws[nws:] == 0x5A).all()) and bool((out[n * H * W:] == 0x5A).all()) and int(status[n]) == -7
    return out[:n * H * W].view(n, H, W).cpu().numpy(), status[:n].cpu().tolist(), intact


@pytest.mark.parametrize('size', list(R.by_size()), ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_case_of_one_size_in_one_call(size):
    """several waves and mixed depths, filters and block types in one launch; the 1x1 group is a call of a single frame"""
    from rmem_ocu_amd import png
    names = R.by_size()[size]
    cs = R.cases()
    lut = cs[names[0]].lut
    assert all((cs[n].lut is None) == (lut is None) for n in names)
    pk = png.PackedPngs([cs[n].png for n in names])
    got = png.decode_label_stack(pk, DEV, lut=lut)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (len(names),) + size
    assert pk.status(DEV).cpu().tolist() == [0] * len(names)
    for k, n in enumerate(names):
        assert torch.equal(got[k].cpu(), torch.from_numpy(expected(n))), n
    bytes_got = png.decode_label_stack([cs[n].png for n in names], DEV, lut=lut)          # from bytes: packed inside
    assert torch.equal(bytes_got, got)


def many_small_files(n):
    hows = ('stored', 'fixed', 'dynamic', 'rle', 'huffman_only')
    labs = [R.noise(8, 9, 1 << (1, 2, 4, 8)[i % 4], 300 + i) for i in range(n)]
    files = [R.build_png(lab, depth=(1, 2, 4, 8)[i % 4], filters=[(i + y) % 5 for y in range(8)], compress_how=hows[i % 5]) for i, lab in enumerate(labs)]
    return labs, files


def test_65_frames_cross_the_chunk():
    from rmem_ocu_amd import png
    labs, files = many_small_files(65)
    assert png.CHUNK == 64
    got = png.decode_label_stack(files, DEV)
    assert torch.equal(got.cpu(), torch.from_numpy(np.stack(labs)))


@pytest.mark.parametrize('size', [(64, 200), (3, 13)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_stale_buffers_and_canaries(size):
    """out pre-filled with 0xA5 and the workspace with 0xFF, then with other fillers: the same labels, nothing written outside"""
    names = R.by_size()[size]
    files = [R.cases()[n].png for n in names]
    want = np.stack([expected(n) for n in names])
    for out_fill, ws_fill in ((0xA5, 0xFF), (0x00, 0x05)):
        got, status, intact = raw_decode(files, None, out_fill, ws_fill)
        assert status == [0] * len(names) and intact
        assert np.array_equal(got, want)


def test_lut():
    from rmem_ocu_amd import png
    names = R.by_size()[(97, 131)]
    lut = np.random.RandomState(2).permutation(256).astype(np.uint8)
    got = png.decode_label_stack([R.cases()[n].png for n in names], DEV, lut=lut)
    for k, n in enumerate(names):
        assert torch.equal(got[k].cpu(), torch.from_numpy(lut[R.cases()[n].label])), n
    on_device = png.decode_label_stack([R.cases()[n].png for n in names], DEV, lut=torch.from_numpy(lut).to(DEV))
    assert torch.equal(on_device, got)
    grey = R.cases()['grey_40x50']
    plain = png.decode_label_stack([grey.png], DEV)
    assert set(np.unique(plain.cpu().numpy()).tolist()) == {0, 255}
    assert set(np.unique(png.decode_label_stack([grey.png], DEV, lut=grey.lut).cpu().numpy()).tolist()) == {0, 1}


@pytest.mark.parametrize('name', [n for n in P.case_names() if not n.startswith('run_') and '480' not in n and '1080' not in n])
def test_round_trip_through_the_encoder(name):
    from rmem_ocu_amd import png
    x = torch.from_numpy(P.case(name)).to(DEV)
    files = png.encode_label_stack(x)
    assert torch.equal(png.decode_label_stack(files, DEV)[0], x)


def test_pillow_480p():
    """the one real-size case: a frame's stream wraps the 32 KiB window many times at the workload's row stride"""
    from rmem_ocu_amd import png
    lab = blobs(480, 854, 11, seed=4)
    assert len(np.unique(lab)) == 11                    # ten objects and the background, none hidden
    data = R._pillow(lab)
    assert np.array_equal(np.array(Image.open(io.BytesIO(data))), lab) and 480 * 855 > 12 * 32768
    got = png.decode_label_stack([data, R._pillow(lab[::-1].copy(), optimize=True)], DEV)
    assert torch.equal(got[0].cpu(), torch.from_numpy(lab)) and torch.equal(got[1].cpu(), torch.from_numpy(lab[::-1].copy()))


def test_corrupt_streams_end_in_their_status_bit():
    """each damaged stream once, in one batch between valid frames: the valid ones decode exactly, a damaged one reports exactly
    its bit and comes out all zero (over a pre-filled out), and nothing is written outside the buffers"""
    cc = R.corrupt_cases()
    lab = R.corrupt_label()
    valid = [R.build_png(lab, compress_how=h) for h in ('dynamic', 'fixed', 'stored')]
    names = list(cc)
    files = [valid[0]] + [cc[n][0] for n in names] + valid[1:]
    want_status = [0] + [cc[n][1] for n in names] + [0, 0]
    got, status, intact = raw_decode(files)
    assert intact
    assert status == want_status, dict(zip(['valid'] + names + ['valid', 'valid'], status))
    for k, st in enumerate(want_status):
        assert np.array_equal(got[k], lab if st == 0 else np.zeros_like(lab)), k


def test_decode_labels_into_does_not_wait_for_the_gpu():
    """stream-ordered: the side stream is kept busy by a device-side spin queued ahead; an event recorded behind the decode is
    still pending when decode_labels_into returns, so the call did not synchronise.  check() does, and reads the status."""
    from rmem_ocu_amd import png
    names = R.by_size()[(64, 200)]
    pk = png.PackedPngs([R.cases()[n].png for n in names])
    want = torch.from_numpy(np.stack([expected(n) for n in names]))
    side = torch.cuda.Stream(DEV)
    out = torch.empty(len(names), 64, 200, dtype=torch.uint8, device=DEV)
    png.decode_labels_into(pk, out, 0, len(names), side)           # first use: device copy of the pack, workspace, code objects
    pk.check(DEV, stream=side)
    assert torch.equal(out.cpu(), want)
    out.fill_(0xA5)
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
    png.decode_labels_into(pk, out[:3], 0, 3, side)
    png.decode_labels_into(pk, out[3:], 3, len(names) - 3, side.cuda_stream)       # a raw handle names the same stream
    done.record(side)
    assert not done.query()
    pk.check(DEV, stream=side)
    assert done.query() and torch.equal(out.cpu(), want)


def test_host_fallback_takes_only_refused_formats():
    from rmem_ocu_amd import png
    from rmem_ocu_amd._lib import RmemError
    lab = blobs(20, 30, 4, seed=17)
    grey16 = io.BytesIO()
    Image.fromarray(lab.astype(np.uint16)).save(grey16, format='PNG')
    files = [R.build_png(lab), grey16.getvalue(), R.build_png(lab[::-1].copy(), depth=2)]
    with pytest.raises(png.PngUnsupported, match='16-bit'):
        png.decode_label_stack(files, DEV)
    got = png.decode_label_stack(files, DEV, host_fallback=True)
    assert torch.equal(got.cpu(), torch.from_numpy(np.stack([lab, lab, lab[::-1]])))
    with pytest.raises(RmemError, match=r'PNG frame 1 failed to decode on the GPU \(status 32: Adler-32 mismatch\)'):    # not handed to the host
        png.decode_label_stack([files[0], R.corrupt_cases()['adler'][0]], DEV, host_fallback=True)


def test_labels_from_pngs_feed_score_clip(tmp_path):
    from rmem_ocu_amd import evaluator
    gts = [blobs(40, 50, 4, seed=60 + (i // 2)) for i in range(6)]
    paths = []
    for i, g in enumerate(gts):
        paths.append(str(tmp_path / f'{i:05d}.png'))
        evaluator.save_mask(g, paths[-1])
    pred = torch.from_numpy(np.stack([shifted_speckled(g, 1, -2, seed=i) for i, g in enumerate(gts)])).to(DEV)
    gt = evaluator.labels_from_pngs(paths, DEV)
    uploaded = torch.from_numpy(np.stack(gts)).to(DEV)
    assert torch.equal(gt, uploaded)
    a, b = evaluator.score_clip(pred, gt), evaluator.score_clip(pred, uploaded)
    assert np.array_equal(a.J, b.J) and np.array_equal(a.F, b.F) and a.JF_mean == b.JF_mean and 0 < a.JF_mean < 1
    first = gt[0].float()[None, None]
    assert tuple(first.shape) == (1, 1, 40, 50) and first.max() == 3
