"""GPU: ubd_extract_objects (rectified patches of the found objects) against the numpy restatement tests/object_patches_oracle.py,
which tests/test_object_patches_host.py pins against Pillow's Image.transform(size, QUAD, data, BILINEAR) bit for bit.  Every
comparison is np.array_equal: no tolerance.  The output buffers are pre-filled with a sentinel and carry guard bytes at both
ends: slots without an object and the guards must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import object_patches_oracle as opo  # noqa: E402
from ubdvss_amd import _lib, NetConfig, Model, ModelRunner, PreprocessingType, extract_objects_on_device  # noqa: E402

pytestmark = pytest.mark.gpu

SENT, GUARD = 0xA5, 64
SENT32 = int(np.frombuffer(bytes([SENT] * 4), np.int32)[0])
SIZES = [(1, 1), (37, 53), (64, 48)]                                    # (rows, cols)
SCALES = [(2.5, 0.75), (1.0, 1.0), (0.5, 1.75)]


def _images(c, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in SIZES]


def _pack(images):
    """one device buffer with image k at a byte offset of +0, +1, +3 from a dword boundary (torch allocations are 256-aligned)"""
    offs, end = [], 0
    for k, a in enumerate(images):
        offs.append((end + 3) // 4 * 4 + (0, 1, 3)[k % 3])
        end = offs[-1] + a.nbytes
    host = np.full(end, 0x5A, np.uint8)
    for o, a in zip(offs, images):
        host[o:o + a.nbytes] = a.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 4 == 0
    return buf, np.array(offs, np.int64), np.array([a.shape[:2] for a in images], np.int32)


def _rotated_rect(cx, cy, w, h, deg):
    t = np.deg2rad(deg)
    ux, uy = np.array([np.cos(t), np.sin(t)]) * w / 2, np.array([-np.sin(t), np.cos(t)]) * h / 2
    pts = [np.array([cx, cy]) + s * ux + r * uy for s, r in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    return [int(round(v)) for p in pts for v in p]


def _quad_kinds(h, w):
    """every kind of quad the kernel can meet, for an image of h x w"""
    return [
        _rotated_rect(w / 2, h / 2, w * 0.6, h * 0.3, 25),                       # rotated rectangles
        _rotated_rect(w / 3, h / 2, w * 0.2, h * 0.7, -40),                      # ... a tall one
        _rotated_rect(0, 0, w * 0.8, h * 0.5, 10),                               # partly outside, negative coordinates
        _rotated_rect(w, h, w * 0.5, h * 0.9, 70),                               # partly outside on the far side
        [w + 9, h + 9, w + 30, h + 9, w + 30, h + 20, w + 9, h + 20],            # wholly outside: all zero
        [-40, -30, -10, -30, -10, -5, -40, -5],                                  # wholly outside, negative
        [w // 2, h // 2] * 4,                                                    # all four corners equal
        [1, 1, w - 1, h - 1, w - 1, h - 1, 1, 1],                                # a zero-area sliver (two pairs)
        [0, 0, w // 3, h // 3, 2 * (w // 3), 2 * (h // 3), w // 2, h // 2],      # ... four collinear points
        [2, 2, 2, h - 2, w - 2, h - 2, w - 2, 2],                                # counter-clockwise order
        [3, 3, 3 + min(w, h) // 2, 3, 3 + min(w, h) // 2, 3 + min(w, h) // 2, 3, 3 + min(w, h) // 2],   # the tie square
        [1, 2, w - 3, 0, w - 1, h - 2, w // 4, h - 1],                           # a general non-rectangular quad
        [w - 2, 1, w // 5, h // 2, 2, h - 1, w - 1, h - 3],                      # ... another, counter-clockwise
    ]


def _call(lib, buf, offs_d, hw_d, c, quads_d, counts_d, n, cap, scales_d, expand, out, ph, pw, pq, src_bytes=None):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.ubd_extract_objects(buf.data_ptr(), buf.numel() if src_bytes is None else src_bytes, offs_d.data_ptr(), hw_d.data_ptr(), c,
                                   quads_d.data_ptr(), counts_d.data_ptr(), n, cap, None if scales_d is None else scales_d.data_ptr(),
                                   expand, out.data_ptr() + GUARD, ph, pw, None if pq is None else pq.data_ptr() + GUARD, st)


def _run_and_check(images, quads, counts, cap, ph, pw, scales, expand, with_pq):
    """one direct call of the C entry point; patches, patch_quads, untouched slots and guards against the oracle"""
    lib = _lib.load()
    n, c = len(images), images[0].shape[2]
    buf, offs, hw = _pack(images)
    offs_d, hw_d = torch.from_numpy(offs).cuda(), torch.from_numpy(hw).cuda()
    quads_d, counts_d = torch.from_numpy(quads).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    scales_d = None if scales is None else torch.from_numpy(np.asarray(scales, np.float64)).cuda()
    pbytes = ph * pw * c
    out = torch.full((2 * GUARD + n * cap * pbytes,), SENT, dtype=torch.uint8, device="cuda")
    pq = torch.full((2 * GUARD + n * cap * 32,), SENT, dtype=torch.uint8, device="cuda") if with_pq else None
    _lib.check(_call(lib, buf, offs_d, hw_d, c, quads_d, counts_d, n, cap, scales_d, expand, out, ph, pw, pq), "ubd_extract_objects")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
    got = got[GUARD:-GUARD].reshape(n, cap, ph, pw, c)
    if with_pq:
        gq = pq.cpu().numpy()
        assert (gq[:GUARD] == SENT).all() and (gq[-GUARD:] == SENT).all()
        gq = gq[GUARD:-GUARD].view(np.int32).reshape(n, cap, 8)
    nonzero = 0
    for i in range(n):
        for j in range(cap):
            if j < min(int(counts[i]), cap):
                want, wq = opo.extract(images[i], quads[i, j], ph, pw, None if scales is None else scales[i], expand)
                assert np.array_equal(got[i, j], want), (i, j, quads[i, j].tolist(), int((got[i, j] != want).sum()))
                nonzero += int(want.any())
                if with_pq:
                    assert gq[i, j].tolist() == wq, (i, j)
            else:
                assert (got[i, j] == SENT).all(), (i, j)
                if with_pq:
                    assert (gq[i, j] == SENT32).all(), (i, j)
    return nonzero, got


PARAMS = [(None, 1.0, False), (SCALES, 1.25, True), (None, 1.25, True), (SCALES, 1.0, False)]


@pytest.mark.parametrize("counts", [[0, 2, 6], [6, 0, 2]])
@pytest.mark.parametrize("ph,pw", [(1, 1), (3, 5), (8, 32)])
@pytest.mark.parametrize("c", [1, 3])
def test_three_images_every_alignment(c, ph, pw, counts):
    """1 x 1, 37 x 53 and 64 x 48 images at byte offsets +0, +1, +3 in one call, cap = 4 and one count above it; (3, 5) patches
    have odd byte counts (every store alignment, tails shorter than four pixels); the second order of the counts puts the
    objects on the 1 x 1 image too"""
    images = _images(c)
    cap = 4
    quads = np.zeros((3, cap, 8), np.int32)
    for i, (h, w) in enumerate(SIZES):
        kinds = _quad_kinds(h, w)
        for j in range(cap):
            quads[i, j] = kinds[(3 * i + 5 * j) % len(kinds)] if (i, j) != (2, 0) else _rotated_rect(w / 2, h / 2, w * 0.7, h * 0.4, 15)
    total = 0
    for scales, expand, with_pq in PARAMS:
        nz, _ = _run_and_check(images, quads, counts, cap, ph, pw, scales, expand, with_pq)
        total += nz
    assert total >= 4                                                   # the comparison covers real pixels


def test_default_patch_size_once():
    images = _images(3)
    quads = np.stack([np.array(_quad_kinds(h, w)[:2], np.int32) for h, w in SIZES])
    nz, _ = _run_and_check(images, quads, [2, 1, 5], 2, 64, 256, SCALES, 1.25, True)
    assert nz >= 3


@pytest.mark.parametrize("c", [1, 3])
def test_every_kind_of_quad(c):
    images = _images(c, seed=11)
    cap = len(_quad_kinds(8, 8))
    quads = np.stack([np.array(_quad_kinds(h, w), np.int32) for h, w in SIZES])
    for scales, expand, with_pq in PARAMS:
        nz, got = _run_and_check(images, quads, [cap] * 3, cap, 6, 17, scales, expand, with_pq)
        assert nz >= 8
        if scales is None and expand == 1.0:
            assert not got[1, 4].any() and not got[1, 5].any()          # wholly outside: all zero (written, not left alone)


def test_graph_capture_equals_the_direct_call():
    lib = _lib.load()
    images = _images(3, seed=5)
    cap, ph, pw = 3, 5, 9
    quads = np.stack([np.array(_quad_kinds(h, w)[:cap], np.int32) for h, w in SIZES])
    buf, offs, hw = _pack(images)
    offs_d, hw_d = torch.from_numpy(offs).cuda(), torch.from_numpy(hw).cuda()
    quads_d, counts_d = torch.from_numpy(quads).cuda(), torch.tensor([3, 1, 2], dtype=torch.int32, device="cuda")
    scales_d = torch.from_numpy(np.asarray(SCALES, np.float64)).cuda()
    nbytes = 2 * GUARD + 3 * cap * ph * pw * 3
    direct = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    pq_direct = torch.full((2 * GUARD + 3 * cap * 32,), SENT, dtype=torch.uint8, device="cuda")
    pq = torch.full((2 * GUARD + 3 * cap * 32,), SENT, dtype=torch.uint8, device="cuda")

    def call(o, q):
        _lib.check(_call(lib, buf, offs_d, hw_d, 3, quads_d, counts_d, 3, cap, scales_d, 1.25, o, ph, pw, q), "ubd_extract_objects")
    call(direct, pq_direct)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(out, pq)                                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # captures on a side stream of its own
        call(out, pq)
    out.fill_(SENT)
    pq.fill_(SENT)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, direct) and torch.equal(pq, pq_direct)
    assert (direct[GUARD:-GUARD] != SENT).any()


def test_refusals_leave_the_output_untouched():
    lib = _lib.load()
    images = _images(3)
    buf, offs, hw = _pack(images)
    offs_d, hw_d = torch.from_numpy(offs).cuda(), torch.from_numpy(hw).cuda()
    quads_d = torch.from_numpy(np.stack([np.array(_quad_kinds(h, w)[:2], np.int32) for h, w in SIZES])).cuda()
    counts_d = torch.tensor([2, 2, 2], dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + 3 * 2 * 4 * 4 * 3,), SENT, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(src=buf.data_ptr(), src_bytes=buf.numel(), src_offsets=offs_d.data_ptr(), src_hw=hw_d.data_ptr(), channels=3,
                quads=quads_d.data_ptr(), counts=counts_d.data_ptr(), n=3, cap=2, scales=None, expand=1.0,
                patches=out.data_ptr() + GUARD, patch_h=4, patch_w=4, patch_quads=None, stream=st)
    bad = [("src", None, "src"), ("src_offsets", None, "src_offsets"), ("src_hw", None, "src_hw"), ("quads", None, "quads"),
           ("counts", None, "counts"), ("patches", None, "patches"), ("n", 0, "n must"), ("n", -1, "n must"), ("cap", 0, "cap must"), ("cap", -5, "cap must"),
           ("patch_h", 0, "patch_h"), ("patch_h", 1025, "patch_h"), ("patch_w", 0, "patch_w"), ("patch_w", 1025, "patch_w"),
           ("channels", 2, "channels"), ("channels", 4, "channels"), ("expand", 0.0, "expand"), ("expand", -1.0, "expand"),
           ("expand", float("inf"), "expand"), ("expand", float("nan"), "expand")]
    for name, value, word in bad:
        args = dict(good)
        args[name] = value
        rc = lib.ubd_extract_objects(*args.values())
        msg = lib.ubd_last_error().decode()
        assert rc != 0, (name, value)
        assert "ubd_extract_objects" in msg and word in msg, (name, value, msg)
    # the block count: n * cap * blocks per patch reaches 2^31 (nothing is launched, so the sizes need no memory behind them)
    for n, cap, ph, pw in ((1 << 16, 1 << 15, 4, 4), (1 << 11, 1 << 10, 1024, 1024), (1 << 20, 1 << 20, 4, 4)):
        args = dict(good, n=n, cap=cap, patch_h=ph, patch_w=pw)
        assert lib.ubd_extract_objects(*args.values()) != 0
        assert "2^31" in lib.ubd_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert lib.ubd_extract_objects(*good.values()) == 0                 # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert (out[GUARD:-GUARD] != SENT).any() and (out[:GUARD] == SENT).all() and (out[-GUARD:] == SENT).all()


def test_an_image_outside_src_bytes_is_empty():
    """The descriptor is merely wrong for the src_bytes given: the buffer really holds all three images, the call is told it ends
    before the last one (and, second case, that an image starts at a negative offset).  The kernel's own range check makes those
    images empty: their patches are written, all zero; the other images are sampled as usual."""
    lib = _lib.load()
    images = _images(3)
    cap, ph, pw = 2, 3, 5
    quads = np.stack([np.array(_quad_kinds(h, w)[:cap], np.int32) for h, w in SIZES])
    buf, offs, hw = _pack(images)
    hw_d, quads_d = torch.from_numpy(hw).cuda(), torch.from_numpy(quads).cuda()
    counts_d = torch.tensor([2, 2, 2], dtype=torch.int32, device="cuda")
    end2 = int(offs[2]) + images[2].nbytes
    for src_bytes, offsets, empty in ((end2 - 1, offs, [2]), (end2, offs, []), (int(offs[2]), offs, [2]),
                                      (end2, np.array([offs[0], -4, offs[2]], np.int64), [1])):
        offs_d = torch.from_numpy(np.ascontiguousarray(offsets)).cuda()
        out = torch.full((2 * GUARD + 3 * cap * ph * pw * 3,), SENT, dtype=torch.uint8, device="cuda")
        _lib.check(_call(lib, buf, offs_d, hw_d, 3, quads_d, counts_d, 3, cap, None, 1.0, out, ph, pw, None, src_bytes=src_bytes),
                   "ubd_extract_objects")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
        got = got[GUARD:-GUARD].reshape(3, cap, ph, pw, 3)
        for i in range(3):
            for j in range(cap):
                want = np.zeros((ph, pw, 3), np.uint8) if i in empty else opo.extract(images[i], quads[i, j], ph, pw)[0]
                assert np.array_equal(got[i, j], want), (src_bytes, i, j)
        assert got[2].any() == (2 not in empty)


def test_python_seam_host_and_device_sources():
    """extract_objects_on_device: a PIL image, a numpy array and a device tensor in one call; empty slots read as 0"""
    from PIL import Image
    rng = np.random.default_rng(3)
    arrays = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((40, 60), (37, 53), (64, 48))]
    sources = [Image.fromarray(arrays[0]), arrays[1], torch.from_numpy(arrays[2]).cuda()]
    cap = 3
    quads = np.stack([np.array(_quad_kinds(*a.shape[:2])[:cap], np.int32) for a in arrays])
    counts = np.array([3, 0, 2], np.int32)
    patches, pq = extract_objects_on_device(sources, torch.from_numpy(quads).cuda(), counts, scales=SCALES, patch_size=(8, 32),
                                            expand=1.25, return_quads=True)
    assert patches.shape == (3, cap, 8, 32, 3) and patches.dtype == torch.uint8 and pq.shape == (3, cap, 8)
    got, gq = patches.cpu().numpy(), pq.cpu().numpy()
    for i in range(3):
        for j in range(cap):
            if j < counts[i]:
                want, wq = opo.extract(arrays[i], quads[i, j], 8, 32, SCALES[i], 1.25)
                assert np.array_equal(got[i, j], want) and gq[i, j].tolist() == wq, (i, j)
            else:
                assert not got[i, j].any() and not gq[i, j].any()
    only = extract_objects_on_device(sources, quads, counts)
    assert only.shape == (3, cap, 64, 256, 3)
    assert np.array_equal(only[0, 1].cpu().numpy(), opo.extract(arrays[0], quads[0, 1], 64, 256)[0])


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


def _check_end_to_end(runner, model, frames, patch_size, expand):
    from PIL import Image
    want_found = runner.predict_images(model, frames)
    found, patches = runner.predict_patches(model, frames, patch_size=patch_size, expand=expand)
    assert [_key(o) for o in found] == [_key(o) for o in want_found]
    for k, im in enumerate(frames):
        raw = np.asarray(im.convert("RGB")) if isinstance(im, Image.Image) else im
        assert patches[k].shape == (len(found[k]), patch_size[0], patch_size[1], 3) and patches[k].dtype == np.uint8
        for j, o in enumerate(found[k]):
            want, _ = opo.extract(raw, o.bbox, patch_size[0], patch_size[1], None, expand)       # no further rescale
            assert np.array_equal(patches[k][j], want), (k, j, list(o.bbox))
    return [len(o) for o in found]


def _frames(sizes, seed):
    """the construction of tests/test_gpu_predict_images.py: textured rectangles at the raw size (RGB), every other one a PIL image"""
    from PIL import Image
    from ubdvss_amd import synthetic
    out = []
    for k, (h, w) in enumerate(sizes):
        hh, ww = -(-h // 4) * 4, -(-w // 4) * 4
        lab = synthetic.rectangle_maps(seed + k, 1, hh // 4, ww // 4)
        a = synthetic.textured_images(seed + 50 + k, lab, 4, 3)[0, :h, :w]
        a = (a.astype(np.int32) * np.array([1.0, 0.8, 0.6])).astype(np.uint8)
        out.append(Image.fromarray(a) if k % 2 else a)
    return out


def test_predict_patches_with_the_golden_detection_weights(golden_dir):
    """The golden detection weights (net_rgb_det.npz) are a random initialisation whose logits stay between -0.5 and 0.05 on these
    frames (fp64 oracle): at pixel_threshold 0.3 (logit -0.85) every pixel is positive and each frame yields one box, its whole
    map -- scaled back by two different ResizeMeta pairs onto two frames of different sizes."""
    from oracle import net_numpy as onet
    d = np.load(os.path.join(golden_dir, "net_rgb_det.npz"))
    cfg = NetConfig(grey=False, fml_compatible=bool(d["fml"]))
    model = Model(cfg)
    model.set_weights(onet.unflatten_weights(d["params"], 3, 0))
    runner = ModelRunner(cfg, pixel_threshold=0.3, max_objects_per_image=16)
    frames = _frames([(100, 180), (140, 90)], 80)
    for size, expand in (((64, 256), 1.0), ((9, 21), 1.25)):
        n_found = _check_end_to_end(runner, model, frames, size, expand)
        assert min(n_found) >= 1, n_found                               # at least one box on each frame


def test_predict_patches_with_a_trained_model():
    """the trained model and frames of tests/test_gpu_predict_images.py: rotated boxes of real detections, grouped by target size"""
    import test_gpu_predict_images as tpi
    cfg = NetConfig(grey=False, preprocessing=PreprocessingType.MOBILENET_LIKE)
    model = tpi._trained_model(cfg, 60)
    runner = ModelRunner(cfg, pixel_threshold=0.5, max_objects_per_image=512)
    frames = _frames([(480, 640), (555, 777), (256, 512), (480, 640)], 83)
    n_found = _check_end_to_end(runner, model, frames, (16, 48), 1.25)
    print("objects per frame:", n_found)
    assert sum(n_found) >= 1, n_found
    f1, p1 = runner.predict_patches(model, frames, patch_size=(16, 48), expand=1.25, batch_size=1)
    f0, p0 = runner.predict_patches(model, frames, patch_size=(16, 48), expand=1.25)
    assert [_key(o) for o in f1] == [_key(o) for o in f0] and all(np.array_equal(a, b) for a, b in zip(p0, p1))
