"""GPU: device bicubic resize (ubd_resize_images; reference SegmapManager._rescale_image_and_markup, segmap_manager.py:135-173,
+ convert('L'), data_generators.py:177) against Pillow itself -- the engine the reference calls -- bit for bit: random source /
target pairs (up- and downscaling, one-pixel sides, one axis unchanged, equal sizes), random pixels and +-255 checkerboards that
drive the ringing into both clip limits, every channel pair, mixed sizes at odd byte offsets in one call, more than one launch's
worth of images, graph capture, and every limit refused with a message."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from ubdvss_amd import _lib, NetConfig, SegmapManager

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (3, 3), (3, 1), (1, 3)]


def _pillow(a, w, h, src_c, dst_c):
    im = Image.fromarray(a[..., 0] if src_c == 1 else a, "L" if src_c == 1 else "RGB")
    if src_c == 1 and dst_c == 3:
        im = im.convert("RGB")
    r = im.resize((w, h), Image.BICUBIC)
    if src_c == 3 and dst_c == 1:
        r = r.convert("L")
    r = np.asarray(r)
    return r[..., None] if r.ndim == 2 else r


def _image(rng, h, w, c):
    if rng.random() < 0.4:                                    # pixel checkerboard (+-255 steps), per channel phase
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([((yy + xx + k) % 2) * 255 for k in range(c)], -1).astype(np.uint8)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def _device_resize(srcs, dst_h, dst_w, src_c, dst_c, misalign=(0, 1, 3), base_shift=0):
    """all sources in one device buffer at offsets that are +0 / +1 / +3 from a 4-byte boundary, base pointer shifted too"""
    lib = _lib.load()
    offs, pos = [], 64
    for k, a in enumerate(srcs):
        pos = (pos + 3) & ~3
        pos += misalign[k % len(misalign)]
        offs.append(pos)
        pos += a.nbytes
    buf = np.zeros(pos + 64, np.uint8)
    for a, o in zip(srcs, offs):
        buf[o:o + a.nbytes] = a.reshape(-1)
    dbuf = torch.from_numpy(buf).cuda()
    hw = np.array([[a.shape[0], a.shape[1]] for a in srcs], np.int32)
    offsets = np.array(offs, np.int64) - base_shift
    out = torch.full((len(srcs), dst_h, dst_w, dst_c), 7, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ubd_resize_images(dbuf.data_ptr() + base_shift, offsets.ctypes.data, hw.ctypes.data, src_c, len(srcs),
                                     out.data_ptr(), dst_h, dst_w, dst_c, stream), "ubd_resize_images")
    return out.cpu().numpy()


def _side(rng, out, special):
    if special == "same":
        return out
    lo, hi = max(1, -(-out // 4)), min(1100, out * 8)          # upscale up to 4x, downscale up to 8x
    return int(rng.integers(lo, hi + 1))


def test_random_pairs_equal_pillow():
    rng = np.random.default_rng(2024)
    n_pairs = 0
    for case in range(72):
        src_c, dst_c = PAIRS[case % 4]
        kind = case % 6
        dst_h = 1 if kind == 1 else int(rng.integers(1, 601))
        dst_w = 1 if kind == 2 else int(rng.integers(1, 601))
        srcs = []
        for k in range(int(rng.integers(2, 5))):
            spec_h = "same" if (kind == 3 and k % 2 == 0) or (kind == 5 and k == 0) else None
            spec_w = "same" if (kind == 4 and k % 2 == 0) or (kind == 5 and k == 0) else None
            h, w = _side(rng, dst_h, spec_h), _side(rng, dst_w, spec_w)
            if k == 1 and kind == 0:
                h = 1                                           # a one-row source
            srcs.append(_image(rng, h, w, src_c))
        got = _device_resize(srcs, dst_h, dst_w, src_c, dst_c, base_shift=case % 3)
        for i, a in enumerate(srcs):
            ref = _pillow(a, dst_w, dst_h, src_c, dst_c)
            assert np.array_equal(got[i], ref), (case, i, a.shape, (dst_h, dst_w), (src_c, dst_c),
                                                 int((got[i] != ref).sum()))
            n_pairs += 1
    assert n_pairs >= 200


@pytest.mark.parametrize("src_c,dst_c", PAIRS)
def test_camera_frames_and_clip_limits(src_c, dst_c):
    """1080p / 720p / 480p to the grey net's sizes, and +-255 checkerboards up- and downscaled (both clip limits reached)."""
    rng = np.random.default_rng(7 + src_c * 3 + dst_c)
    srcs = [_image(rng, 1080, 1920, src_c), _image(rng, 720, 1280, src_c)]
    got = _device_resize(srcs, 256, 512, src_c, dst_c)
    for i, a in enumerate(srcs):
        assert np.array_equal(got[i], _pillow(a, 512, 256, src_c, dst_c))
    yy, xx = np.mgrid[0:37, 0:53]
    board = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], src_c, -1)
    for dh, dw in ((148, 212), (9, 13), (37, 100)):
        got = _device_resize([board], dh, dw, src_c, dst_c)[0]
        ref = _pillow(board, dw, dh, src_c, dst_c)
        assert np.array_equal(got, ref)
    up = _pillow(board, 212, 148, src_c, src_c)
    assert up.min() == 0 and up.max() == 255


def test_more_images_than_one_launch():
    rng = np.random.default_rng(99)
    srcs = [_image(rng, int(rng.integers(1, 90)), int(rng.integers(1, 90)), 3) for _ in range(150)]
    got = _device_resize(srcs, 24, 40, 3, 1)
    for i, a in enumerate(srcs):
        assert np.array_equal(got[i], _pillow(a, 40, 24, 3, 1)), i


@pytest.mark.parametrize("src_c,dst_c", [(3, 3), (1, 1)])
def test_extreme_ratios_and_pass_order(src_c, dst_c):
    """downscales by hundreds (tap tables recomputed per use instead of stored), one-pixel targets, and the pass order: Pillow
    runs images more than 100 times as tall as wide vertical first when they shrink vertically (at 100 times: horizontal first)"""
    rng = np.random.default_rng(5)
    cases = (((3000, 40), (1, 7)), ((16, 4000), (5, 1)), ((2, 2), (1, 1)), ((1, 1), (9, 7)), ((607, 2), (474, 1)),
             ((201, 2), (200, 3)), ((200, 2), (199, 1)), ((2000, 20), (1000, 5)), ((2000, 19), (1000, 5)), ((5000, 7), (300, 40)),
             ((401, 4), (402, 2)), ((2, 400), (1, 300)))
    for (h, w), (dh, dw) in cases:
        a = _image(rng, h, w, src_c)
        assert np.array_equal(_device_resize([a], dh, dw, src_c, dst_c)[0], _pillow(a, dw, dh, src_c, dst_c)), (h, w, dh, dw)
    srcs = [_image(rng, h, w, src_c) for h, w in ((900, 8), (1000, 300), (700, 7), (60, 500))]     # both orders in one launch
    got = _device_resize(srcs, 50, 30, src_c, dst_c)
    for i, a in enumerate(srcs):
        assert np.array_equal(got[i], _pillow(a, 30, 50, src_c, dst_c)), i


def test_graph_capture_replays_the_same_bytes():
    lib = _lib.load()
    rng = np.random.default_rng(11)
    srcs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((300, 500, 3), (201, 333, 3), (64, 64, 3))]
    offs = np.array([0, srcs[0].nbytes + 1, srcs[0].nbytes + srcs[1].nbytes + 2], np.int64)
    buf = torch.zeros(int(offs[-1]) + srcs[2].nbytes, dtype=torch.uint8, device="cuda")
    for a, o in zip(srcs, offs):
        buf[int(o):int(o) + a.nbytes] = torch.from_numpy(a.reshape(-1)).cuda()
    hw = np.array([a.shape[:2] for a in srcs], np.int32)
    out = torch.zeros((3, 128, 160, 1), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def call():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.ubd_resize_images(buf.data_ptr(), offs.ctypes.data, hw.ctypes.data, 3, 3, out.data_ptr(), 128, 160, 1, st),
                   "ubd_resize_images")
    with torch.cuda.stream(s):
        call()                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, a in enumerate(srcs):
        assert np.array_equal(got[i], _pillow(a, 160, 128, 3, 1))


def test_limits_are_refused_with_a_message():
    lib = _lib.load()
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    ok_off, ok_hw = np.zeros(2, np.int64), np.full(4, 4, np.int32)

    def call(offs=ok_off, hw=ok_hw, src_c=1, n=1, dh=2, dw=2, dc=1, s=None, d=None):
        return lib.ubd_resize_images(src.data_ptr() if s is None else s, offs.ctypes.data, hw.ctypes.data, src_c, n,
                                     dst.data_ptr() if d is None else d, dh, dw, dc, None)
    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(n=0), dict(src_c=2), dict(dc=0), dict(dh=0), dict(dw=8193), dict(hw=np.array([0, 4], np.int32)),
           dict(hw=np.array([4, 16385], np.int32)), dict(offs=np.array([-1], np.int64)), dict(dh=8192, dw=8192, dc=3, n=11),
           dict(s=0), dict(d=0)]
    for kw in bad:
        n = kw.get("n", 1)
        if "hw" not in kw and n > 1:
            kw["hw"], kw["offs"] = np.full(2 * n, 4, np.int32), np.zeros(n, np.int64)
        assert call(**kw) != 0, kw
        assert lib.ubd_last_error().decode().startswith("ubd_resize_images"), kw
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[4:] == 9).all()                  # nothing was launched for a refused call


def test_python_entry_point_takes_every_input_form():
    """rescale_images_on_device: PIL (via convert('RGB')), numpy HxW / HxWx3 and device tensors in one call, the MetaInfo
    scales, and a ValueError when the target sizes differ."""
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (700, 1300), dtype=np.uint8)
    small = rng.integers(0, 256, (480, 900, 3), dtype=np.uint8)
    images = [Image.fromarray(rgb), grey, torch.from_numpy(small).cuda(), Image.fromarray(grey)]
    for cfg in (NetConfig(), NetConfig(grey=False)):
        x, metas = SegmapManager.rescale_images_on_device(images, cfg)
        assert x.shape == (4, 256, 512, 1 if cfg.is_grey() else 3)
        got = x.cpu().numpy()
        for i, a in enumerate((rgb, grey, small, grey)):
            im = Image.fromarray(a).convert("RGB").resize((512, 256), Image.BICUBIC)
            ref = np.asarray(im.convert("L"))[..., None] if cfg.is_grey() else np.asarray(im)
            assert np.array_equal(got[i], ref), i
            assert (metas[i].xscale, metas[i].yscale) == (a.shape[1] / 512, a.shape[0] / 256)
    with pytest.raises(ValueError, match="target size"):
        SegmapManager.rescale_images_on_device([rgb, rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)], NetConfig())
