"""GPU JPEG decode (rmem_jpeg_*, rmem_ocu_amd/jpeg.py) on the MI355X: coefficients equal the numpy restatement, RGB equals Pillow
bit for bit, corrupted streams are reported, and the slots fed JpegClips give the masks of the same slots fed Pillow-decoded
pinned uint8 frames."""
import io

import numpy as np
import pytest
import torch

PIL = pytest.importorskip('PIL')
from PIL import Image  # noqa: E402

import jpeg_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SUB = {'444': 0, '422': 1, '420': 2}


def encode(a, mode, quality=90, **kw):
    b = io.BytesIO()
    if mode == 'L':
        Image.fromarray(a[..., 0]).save(b, 'JPEG', quality=quality, **kw)
    else:
        Image.fromarray(a).save(b, 'JPEG', quality=quality, subsampling=SUB[mode], **kw)
    return b.getvalue()


def image(h, w, seed=0, noise=40):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 4) % 256], -1)
    return np.clip(smooth + rs.randint(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))


def gpu_decode_list(datas, **kw):
    from rmem_ocu_amd import jpeg
    p = jpeg.PackedJpegs(datas)
    outs = [torch.empty(h, w, 3, dtype=torch.uint8, device=DEV) for h, w in p.sizes]
    p.decode_into(outs, 0, len(datas), **kw)
    torch.cuda.synchronize()
    return p, [o.cpu().numpy() for o in outs]


def test_coefficients_equal_restatement():
    from rmem_ocu_amd import jpeg
    datas = [encode(image(17, 33, 1), 'L', 90), encode(image(40, 72, 2), '444', 50), encode(image(33, 47, 3), '422', 95),
             encode(image(64, 96, 4), '420', 100), encode(image(70, 130, 5), '420', 90, restart_marker_blocks=3),
             encode(image(48, 80, 6), '420', 75, optimize=True, restart_marker_rows=1)]
    p = jpeg.PackedJpegs(datas)
    got = p.coefficients(DEV)
    p.check(DEV)
    for d, g in zip(datas, got):
        ref = jpeg_ref.decode_coefficients(jpeg_ref.parse(d))
        assert np.array_equal(g.cpu().numpy(), ref)


def test_rgb_equals_pillow_mixed_batch():
    rs = np.random.RandomState(7)
    datas = []
    for mode in ('L', '444', '422', '420'):
        for hw in ((1, 1), (7, 9), (17, 33), (64, 96)):
            datas.append(encode(image(*hw, seed=len(datas)), mode, int(rs.choice([50, 90, 100]))))
    datas += [encode(image(481, 853, 11), '420', 90), encode(image(480, 854, 12), '420', 95, optimize=True),
              encode(image(1080, 1920, 13), '420', 90), encode(image(481, 853, 14), '422', 90, restart_marker_rows=1),
              encode(image(200, 301, 15), '444', 95, restart_marker_blocks=7), encode(image(99, 131, 16), 'L', 90, optimize=True),
              encode(image(480, 854, 17), '420', 90, restart_marker_blocks=1)]
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    p, outs = gpu_decode_list(datas, stats=stats)
    p.check(DEV)
    for k, (d, o) in enumerate(zip(datas, outs)):
        assert np.array_equal(o, pillow(d)), k
    assert int(stats[0]) >= 1


@pytest.mark.parametrize('mode', ['444', '420'])
def test_noise_q100_default_and_forced_fallback(mode):
    rs = np.random.RandomState(21)
    datas = [encode(rs.randint(0, 256, (240, 320, 3)).astype(np.uint8), mode, 100),
             encode(rs.randint(0, 256, (97, 203, 3)).astype(np.uint8), mode, 100, restart_marker_rows=2)]
    for kw in ({}, {'sync_rounds': 0}, {'force_fallback': True}):
        stats = torch.zeros(2, dtype=torch.int32, device=DEV)
        p, outs = gpu_decode_list(datas, stats=stats, **kw)
        p.check(DEV)
        for d, o in zip(datas, outs):
            assert np.array_equal(o, pillow(d)), kw
        if kw.get('force_fallback'):
            assert int(stats[1]) == sum(int(x.nunits) for x in p.descs)


def _corrupted(good):
    """good with garbage in its entropy-coded segment (no FF bytes: the markers stay valid) that the restatement rejects (an
    invalid code on the real decode path)"""
    from rmem_ocu_amd import jpeg
    a, b = jpeg.parse(good).scan_range
    for seed in range(100):
        d = bytearray(good)
        rs = np.random.RandomState(seed)
        pos = a + (b - a) // 3
        for k in range(48):
            if d[pos + k - 1] != 0xFF:
                d[pos + k] = int(rs.randint(0, 255))
        d = bytes(d)
        try:
            jpeg_ref.decode_coefficients(jpeg_ref.parse(d))
        except jpeg_ref.DecodeError:
            return d
    pytest.fail('no corruption the restatement rejects')


def test_corrupted_entropy_bytes_give_nonzero_status():
    from rmem_ocu_amd import jpeg
    from rmem_ocu_amd._lib import RmemError
    d = _corrupted(encode(image(120, 160, 9), '420', 90))
    jpeg.parse(d)                                        # headers still parse
    with pytest.raises(RmemError, match='failed to decode'):
        jpeg.decode([d], DEV)
    clip = jpeg.JpegClip([d, encode(image(120, 160, 10), '420', 90)])
    jpeg.decode(clip, DEV, check=False)
    st = clip.status(DEV).cpu().tolist()
    assert st[0] != 0 and st[1] == 0


def test_host_fallback_for_progressive():
    from rmem_ocu_amd import jpeg
    from rmem_ocu_amd._lib import RmemError
    b = io.BytesIO()
    Image.fromarray(image(30, 50, 2)).save(b, 'JPEG', progressive=True)
    with pytest.raises(RmemError, match='progressive'):
        jpeg.decode([b.getvalue()], DEV)
    out = jpeg.decode([b.getvalue()], DEV, host_fallback=True)
    assert np.array_equal(out[0].cpu().numpy(), pillow(b.getvalue()))


def test_gpu_decode_then_ingest_equals_pillow_then_ingest():
    from rmem_ocu_amd import jpeg, ops
    datas = [encode(image(481, 853, 30 + k), '420', 90) for k in range(3)]
    rgb = jpeg.decode(datas, DEV)
    ref = torch.from_numpy(np.stack([pillow(d) for d in datas])).to(DEV)
    assert torch.equal(rgb, ref)
    H, W = 465, 833
    a = torch.empty(3, 3, H, W, device=DEV)
    r = torch.empty(3, 3, H, W, device=DEV)
    ops.run([ops.ingest_rgb8(rgb[k], Hs=481, Ws=853, Hd=H, Wd=W, out_chw=a[k]) for k in range(3)])
    ops.run([ops.ingest_rgb8(ref[k], Hs=481, Ws=853, Hd=H, Wd=W, out_chw=r[k]) for k in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(a, r)


def _jpeg_clip_frames(seed, n, quality=90):
    """A synthetic clip as JPEG bytes (160 x 192, 4:2:0) and the same frames decoded by Pillow into pinned uint8."""
    import torch.nn.functional as F
    from rmem_ocu_amd.synth import make_clip
    frames, mask = make_clip(seed, n, 161, 193, 2)
    vid = F.interpolate(frames, size=(160, 192), mode='bilinear', align_corners=False)
    u8 = (vid * 40.0 + 128.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    datas = [encode(u8[k], '420', quality) for k in range(n)]
    dec = torch.from_numpy(np.stack([pillow(d) for d in datas])).contiguous().pin_memory()
    return datas, dec, mask


def _engine(former, latter, gap):
    from rmem_ocu_amd import build_engine, build_vos_model, get_config
    from rmem_ocu_amd.weights import synth_state_dict
    cfg = get_config('pre_vost', 'test', 'r50_aotl')
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = former, latter
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0))
    return build_engine(cfg.MODEL_ENGINE, phase='eval', aot_model=model, gpu_id=0, long_term_mem_gap=gap).eval()


def test_clip_slot_from_jpeg_clip():
    from rmem_ocu_amd.clip_runner import ClipSlot
    from rmem_ocu_amd.jpeg import JpegClip
    datas, dec, mask = _jpeg_clip_frames(9, 11)
    out = []
    for src in (dec, JpegClip(datas)):
        eng = _engine(1, 2, 2)
        eng.set_async(use_graphs=True)
        slot = ClipSlot(eng, (160, 192), DEV, lookahead=4)
        slot.start(src, mask.to(DEV), 2)
        while not slot.done:
            slot.step()
        eng.synchronize()
        if isinstance(src, JpegClip):
            src.check(DEV)
        out.append(slot.labels[:11].cpu().numpy().copy())
    assert np.array_equal(out[0][1:], out[1][1:])


def test_group_slot_from_jpeg_clips():
    from rmem_ocu_amd import build_vos_model, get_config
    from rmem_ocu_amd.clip_runner import GroupSlot
    from rmem_ocu_amd.jpeg import JpegClip
    from rmem_ocu_amd.networks.engines.group_engine import GroupEngine
    from rmem_ocu_amd.weights import synth_state_dict
    B, n = 2, 9
    cfg = get_config('pre_vost', 'test', 'r50_aotl')
    cfg.FORMER_MEM_LEN, cfg.LATTER_MEM_LEN = 1, 2
    model = build_vos_model(cfg.MODEL_VOS, cfg).cuda(0)
    model.load_state_dict(synth_state_dict(0))
    clips = [_jpeg_clip_frames(60 + c, n) for c in range(B)]
    masks = [m.to(DEV) for _, _, m in clips]
    out = []
    for la in (2, 1):
        for src in ([d for _, d, _ in clips], [JpegClip(j) for j, _, _ in clips]):
            ge = GroupEngine(model, B, 0, 5, lookahead=la)
            gs = GroupSlot(ge, (160, 192), DEV)
            gs.start(src, masks, 2)
            while not gs.done:
                gs.step()
            ge.synchronize()
            for s in src:
                if isinstance(s, JpegClip):
                    s.check(DEV)
            out.append(gs.labels[:, :n].cpu().numpy().copy())
    assert np.array_equal(out[0][:, 1:], out[1][:, 1:])
    assert np.array_equal(out[2][:, 1:], out[3][:, 1:])


def test_frames_from_jpegs_feeds_the_evaluator(tmp_path):
    from rmem_ocu_amd import ops
    from rmem_ocu_amd.evaluator import frames_from_jpegs
    from rmem_ocu_amd.synth import network_size
    datas = [encode(image(300, 500, 40 + k), '420', 90) for k in range(3)]
    paths = []
    for k, d in enumerate(datas):
        p = tmp_path / f'{k:05d}.jpg'
        p.write_bytes(d)
        paths.append(str(p))
    got = frames_from_jpegs(paths, DEV)
    H, W = network_size(300, 500)
    assert tuple(got.shape) == (3, 3, H, W)
    ref = torch.from_numpy(np.stack([pillow(d) for d in datas])).to(DEV)
    want = torch.empty_like(got)
    ops.run([ops.ingest_rgb8(ref[k], Hs=300, Ws=500, Hd=H, Wd=W, out_chw=want[k]) for k in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert tuple(frames_from_jpegs(datas, DEV, scale=1.3).shape) == (3, 3) + network_size(300, 500, scale=1.3)


def test_decode_on_a_side_stream_checks_that_stream_and_chunks():
    """decode(stream=side) allocates and decodes on the side stream, synchronises it before reading the status words, and
    decodes more than jpeg.CHUNK frames in several calls."""
    from rmem_ocu_amd import jpeg
    from rmem_ocu_amd._lib import RmemError
    datas = [encode(image(24, 40, 70 + k), '420', 90) for k in range(jpeg.CHUNK + 5)]
    side = torch.cuda.Stream(DEV)
    torch.cuda.current_stream(DEV).synchronize()
    out = jpeg.decode(datas, DEV, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.stack([pillow(d) for d in datas]))
    bad = _corrupted(encode(image(120, 160, 9), '420', 90))
    with pytest.raises(RmemError, match='failed to decode'):
        jpeg.decode([bad], DEV, stream=side.cuda_stream)


def test_slots_report_a_corrupt_jpeg_frame():
    """A corrupt frame behind valid headers is not turned into masks silently: check_frames() raises, and so does the next
    start()."""
    from rmem_ocu_amd.clip_runner import ClipSlot
    from rmem_ocu_amd.jpeg import JpegClip
    from rmem_ocu_amd._lib import RmemError
    datas, dec, mask = _jpeg_clip_frames(19, 5)
    bad = list(datas)
    bad[3] = _corrupted(datas[3])
    eng = _engine(1, 2, 2)
    slot = ClipSlot(eng, (160, 192), DEV, lookahead=2)
    slot.start(JpegClip(bad), mask.to(DEV), 2)
    while not slot.done:
        slot.step()
    with pytest.raises(RmemError, match='frame 3'):
        slot.check_frames()
    with pytest.raises(RmemError, match='frame 3'):
        slot.start(JpegClip(datas), mask.to(DEV), 2)
    slot.frames = None                                   # the corrupt clip was reported: go on with a clean one
    slot.start(JpegClip(datas), mask.to(DEV), 2)
    while not slot.done:
        slot.step()
    slot.check_frames()
