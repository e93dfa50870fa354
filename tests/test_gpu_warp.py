"""GPU: ubd_warp_images (csrc/warp.hip; the image half of the reference's augmentation.py:50-85) against Pillow itself -- the
engine the reference calls -- bit for bit, np.array_equal, no tolerance, no excluded pixels: Image.rotate(angle, BILINEAR,
expand=True) and Image.transform(size, PERSPECTIVE, coeffs, BILINEAR) on random L / RGB images with sides from 1 to ~1100
(one-pixel rows and columns among them), random pixels and +-255 checkerboards, angles across (-45, 45) with 0 and tiny ones,
perspective coefficients across the reference's box and at its corners, sources at byte offsets +0 / +1 / +3 from a dword
boundary (destinations at +0 / +2), several sizes in one call, more images than one launch takes; the quarter turns and crops
(signed strided views) against Image.transpose / Image.crop; 1080p and 720p frames once per mode; graph capture; every limit
refused with a message."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from ubdvss_amd import _lib
from ubdvss_amd import augmentation as aug

pytestmark = pytest.mark.gpu

COPY, AFFINE, PERSPECTIVE = 0, 1, 2
MEAN, HALF = aug.PERSPECTIVE_MEAN, aug.PERSPECTIVE_HALF


def _image(rng, h, w, c):
    if rng.random() < 0.35:                                   # pixel checkerboard (+-255 steps), per channel phase
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([((yy + xx + k) % 2) * 255 for k in range(c)], -1).astype(np.uint8)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def _pil(a):
    return Image.fromarray(a[..., 0] if a.shape[2] == 1 else a, "L" if a.shape[2] == 1 else "RGB")


def _arr(im):
    r = np.asarray(im)
    return r[..., None] if r.ndim == 2 else r


class Job:
    """one image of a call: source array, the view edits (crop window / quarter turns) applied to it, mode, coefficients,
    destination (w, h)"""

    def __init__(self, a, mode, coeffs=None, dst=None, edits=()):
        self.a, self.mode, self.coeffs, self.edits = a, mode, coeffs, edits
        v = aug._View(0, a.shape[1], a.shape[0], a.shape[2], None)
        for kind, arg in edits:
            v.crop(*arg) if kind == "crop" else v.quarter(arg)
        self.view = v
        self.dst = (v.w, v.h) if dst is None else dst


def _device_warp(jobs, c, misalign=(0, 1, 3), dst_misalign=(0, 2), base_shift=0, stream=None):
    """all sources in one device buffer at offsets +0 / +1 / +3 from a 4-byte boundary, destinations at +0 / +2, guard bytes
    between the destinations checked"""
    lib = _lib.load()
    offs, pos = [], 64
    for k, j in enumerate(jobs):
        pos = ((pos + 3) & ~3) + misalign[k % len(misalign)]
        offs.append(pos)
        pos += j.a.nbytes
    buf = np.zeros(pos + 64, np.uint8)
    for j, o in zip(jobs, offs):
        buf[o:o + j.a.nbytes] = j.a.reshape(-1)
    dbuf = torch.from_numpy(buf).cuda()
    doffs, pos = [], 16
    for k, j in enumerate(jobs):
        pos = ((pos + 3) & ~3) + dst_misalign[k % len(dst_misalign)]
        doffs.append(pos)
        pos += j.dst[0] * j.dst[1] * c + 8
    out = torch.full((pos + 16,), 7, dtype=torch.uint8, device="cuda")
    descs = np.zeros(len(jobs), aug.WARP_DESC)
    for k, j in enumerate(jobs):
        d, v = descs[k], j.view
        d["src_offset"], d["dst_offset"] = offs[k] + v.ptr - base_shift, doffs[k]
        d["src_xpitch"], d["src_ypitch"], d["src_w"], d["src_h"] = v.xp, v.yp, v.w, v.h
        d["dst_w"], d["dst_h"], d["mode"] = j.dst[0], j.dst[1], j.mode
        if j.coeffs is not None:
            d["coeffs"][:len(j.coeffs)] = j.coeffs
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ubd_warp_images(dbuf.data_ptr() + base_shift, dbuf.numel() - base_shift, out.data_ptr(), out.numel(),
                                   descs.ctypes.data, c, len(jobs), st), "ubd_warp_images")
    o = out.cpu().numpy()
    written = np.zeros(o.size, bool)
    res = []
    for j, p in zip(jobs, doffs):
        n = j.dst[0] * j.dst[1] * c
        res.append(o[p:p + n].reshape(j.dst[1], j.dst[0], c))
        written[p:p + n] = True
    assert (o[~written] == 7).all(), "bytes outside the destinations were written"
    return res


def _rotate_job(a, angle):
    kind, matrix, size = aug.rotate_matrix_and_size(angle, (a.shape[1], a.shape[0]))
    if kind == "copy":                                       # Image.rotate(0) copies; the kernel is given the identity matrix
        return Job(a, AFFINE, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], size), a
    assert kind == "affine"
    ref = _arr(_pil(a).rotate(angle, Image.BILINEAR, expand=True))
    assert ref.shape[:2] == (size[1], size[0])
    return Job(a, AFFINE, matrix, size), ref


def _perspective_job(a, coeffs, dst=None):
    dst = (a.shape[1], a.shape[0]) if dst is None else dst
    return Job(a, PERSPECTIVE, list(coeffs), dst), _arr(_pil(a).transform(dst, Image.PERSPECTIVE, list(coeffs), Image.BILINEAR))


def _check(jobs_refs, c, tag, **kw):
    got = _device_warp([j for j, _ in jobs_refs], c, **kw)
    for i, ((j, ref), g) in enumerate(zip(jobs_refs, got)):
        assert g.shape == ref.shape, (tag, i, g.shape, ref.shape)
        assert np.array_equal(g, ref), (tag, i, j.a.shape, j.mode, j.coeffs, j.dst, f"{int((g != ref).sum())} bytes differ")
    return len(got)


def _side(rng, kind):
    return 1 if kind else int(rng.integers(1, 1101)) if rng.random() < 0.3 else int(rng.integers(1, 200))


def test_random_pairs_equal_pillow():
    rng = np.random.default_rng(2025)
    special_angles = [0.0, 1e-9, -1e-6, 1e-3, -0.01, 44.999999, -44.999999, 45.0, -45.0, 0.5, -30.0, 17.25]
    corners = [MEAN + HALF * np.where((k >> np.arange(8)) & 1, 1, -1) for k in range(0, 256, 17)]
    corners += [MEAN + HALF, MEAN - HALF]
    n_pairs = 0
    for case in range(72):
        c = 1 if case % 2 else 3
        items = []
        for k in range(int(rng.integers(2, 5))):
            h = _side(rng, case % 9 == 1 and k == 0)          # one-pixel rows
            w = _side(rng, case % 9 == 2 and k == 0)          # one-pixel columns
            if case % 9 == 3 and k == 0:
                h = w = 1
            a = _image(rng, h, w, c)
            if (case + k) % 2 == 0:
                n_special = case // 2 * 4 + k
                angle = special_angles[n_special % len(special_angles)] if n_special < 2 * len(special_angles) else float(rng.uniform(-45, 45))
                items.append(_rotate_job(a, angle))
            else:
                n_corner = case // 2 * 4 + k
                coeffs = corners[n_corner % len(corners)] if n_corner < 2 * len(corners) else rng.uniform(MEAN - HALF, MEAN + HALF)
                dst = None if k % 3 else (int(rng.integers(1, 300)), int(rng.integers(1, 300)))   # Pillow takes any output size
                items.append(_perspective_job(a, coeffs, dst))
        n_pairs += _check(items, c, case, base_shift=case % 3)
    assert n_pairs >= 200


@pytest.mark.parametrize("c", [1, 3])
def test_camera_frames_once_per_mode(c):
    rng = np.random.default_rng(40 + c)
    frames = [_image(rng, 1080, 1920, c), _image(rng, 720, 1280, c)]
    _check([_rotate_job(frames[0], 31.7), _rotate_job(frames[1], -12.3)], c, "rotate")
    _check([_perspective_job(frames[0], rng.uniform(MEAN - HALF, MEAN + HALF)), _perspective_job(frames[1], MEAN + HALF)], c, "perspective")
    turned = [(Job(f, COPY, edits=(("quarter", ang),)), _arr(_pil(f).rotate(ang, Image.BILINEAR, expand=True)))
              for f, ang in zip(frames, (90, 180))]
    _check(turned, c, "copy")


def test_quarter_turns_and_crops_are_exact_views():
    rng = np.random.default_rng(8)
    tr = {90: Image.ROTATE_90, 180: Image.ROTATE_180, 270: Image.ROTATE_270}
    n = 0
    for case in range(24):
        c = 1 if case % 2 else 3
        items = []
        for k in range(4):
            h, w = (1, int(rng.integers(1, 40))) if case == 5 and k == 0 else (int(rng.integers(1, 260)), int(rng.integers(1, 260)))
            a = _image(rng, h, w, c)
            im = _pil(a)
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            x1, y1 = int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))
            ang = (90, 180, 270)[(case + k) % 3]
            kind = (case + k) % 5
            if kind == 0:                                    # a quarter turn alone (as Image.rotate does it with expand=True)
                items.append((Job(a, COPY, edits=(("quarter", ang),)), _arr(im.rotate(ang, Image.BILINEAR, expand=True))))
            elif kind == 1:                                  # a crop alone, from a float box
                box = (x0 + 0.3, y0 - 0.4, x1 - 0.2, y1 + 0.49)
                items.append((Job(a, COPY, edits=(("crop", aug.crop_window(box)),)), _arr(im.crop(box))))
            elif kind == 2:                                  # crop, then turn, then crop again
                im2 = im.crop((x0, y0, x1, y1)).transpose(tr[ang])
                u0, v0 = int(rng.integers(0, im2.size[0])), int(rng.integers(0, im2.size[1]))
                win2 = (u0, v0, im2.size[0], im2.size[1])
                items.append((Job(a, COPY, edits=(("crop", (x0, y0, x1, y1)), ("quarter", ang), ("crop", win2))), _arr(im2.crop(win2))))
            elif kind == 3:                                  # a perspective pass that reads through crop + turn
                im2 = im.crop((x0, y0, x1, y1)).transpose(tr[ang])
                coeffs = rng.uniform(MEAN - HALF, MEAN + HALF).tolist()
                items.append((Job(a, PERSPECTIVE, coeffs, edits=(("crop", (x0, y0, x1, y1)), ("quarter", ang))),
                              _arr(im2.transform(im2.size, Image.PERSPECTIVE, coeffs, Image.BILINEAR))))
            else:                                            # a rotation that reads through a turn
                im2 = im.transpose(tr[ang])
                angle = float(rng.uniform(-45, 45))
                _, matrix, size = aug.rotate_matrix_and_size(angle, im2.size)
                items.append((Job(a, AFFINE, matrix, size, edits=(("quarter", ang),)), _arr(im2.rotate(angle, Image.BILINEAR, expand=True))))
        n += _check(items, c, case, base_shift=case % 2)
    assert n == 96


def test_more_images_than_one_launch():
    rng = np.random.default_rng(77)
    items = []
    for k in range(75):
        a = _image(rng, int(rng.integers(1, 70)), int(rng.integers(1, 70)), 3)
        items.append(_rotate_job(a, float(rng.uniform(-45, 45))) if k % 2 else _perspective_job(a, rng.uniform(MEAN - HALF, MEAN + HALF)))
    assert _check(items, 3, "launches") == 75


def test_graph_capture_replays_the_same_bytes():
    lib = _lib.load()
    rng = np.random.default_rng(12)
    srcs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((300, 500, 3), (201, 333, 3), (64, 64, 3))]
    jobs = [_rotate_job(srcs[0], 20.5), _perspective_job(srcs[1], MEAN - HALF), _rotate_job(srcs[2], -44.0)]
    offs = np.array([0, srcs[0].nbytes + 1, srcs[0].nbytes + srcs[1].nbytes + 2], np.int64)
    buf = torch.zeros(int(offs[-1]) + srcs[2].nbytes, dtype=torch.uint8, device="cuda")
    for a, o in zip(srcs, offs):
        buf[int(o):int(o) + a.nbytes] = torch.from_numpy(a.reshape(-1)).cuda()
    descs = np.zeros(3, aug.WARP_DESC)
    pos = 0
    for k, (j, _) in enumerate(jobs):
        d = descs[k]
        d["src_offset"], d["dst_offset"] = offs[k], pos
        d["src_xpitch"], d["src_ypitch"], d["src_w"], d["src_h"] = 3, j.a.shape[1] * 3, j.a.shape[1], j.a.shape[0]
        d["dst_w"], d["dst_h"], d["mode"] = j.dst[0], j.dst[1], j.mode
        d["coeffs"][:len(j.coeffs)] = j.coeffs
        pos += (j.dst[0] * j.dst[1] * 3 + 3) & ~3
    out = torch.zeros(pos, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def call():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.ubd_warp_images(buf.data_ptr(), buf.numel(), out.data_ptr(), out.numel(), descs.ctypes.data, 3, 3, st), "ubd_warp_images")
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
    for k, (j, ref) in enumerate(jobs):
        p = int(descs[k]["dst_offset"])
        assert np.array_equal(got[p:p + ref.size].reshape(ref.shape), ref), k


def test_limits_are_refused_with_a_message():
    lib = _lib.load()
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), 9, dtype=torch.uint8, device="cuda")

    def desc(**kw):
        d = np.zeros(kw.pop("count", 1), aug.WARP_DESC)
        d["src_xpitch"], d["src_ypitch"], d["src_w"], d["src_h"], d["dst_w"], d["dst_h"], d["mode"] = 1, 4, 4, 4, 4, 4, AFFINE
        d["coeffs"][:, :6] = [1, 0, 0, 0, 1, 0]
        for k, v in kw.items():
            d[k] = v
        return d

    def call(d, c=1, n=None, s=None, t=None, sb=256, db=256, null_descs=False):
        return lib.ubd_warp_images(src.data_ptr() if s is None else s, sb, dst.data_ptr() if t is None else t, db,
                                   None if null_descs else d.ctypes.data, c, len(d) if n is None else n, None)
    assert call(desc()) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[16:] == 9).all()
    dst.fill_(9)
    nan = desc()
    nan["coeffs"][0, 3] = np.nan
    inf = desc(mode=PERSPECTIVE)
    inf["coeffs"][0, 7] = np.inf
    bad = [dict(d=desc(), n=0), dict(d=desc(), c=2), dict(d=desc(), c=4), dict(d=desc(), s=0), dict(d=desc(), t=0),
           dict(d=desc(), null_descs=True), dict(d=desc(mode=3)), dict(d=desc(mode=-1)), dict(d=desc(src_w=0)), dict(d=desc(src_h=16385)),
           dict(d=desc(dst_w=0)), dict(d=desc(dst_h=16385)),
           dict(d=desc(mode=COPY, dst_w=5)), dict(d=desc(src_offset=-1)), dict(d=desc(src_offset=241)),
           dict(d=desc(src_xpitch=-1)), dict(d=desc(src_ypitch=-4)), dict(d=desc(src_ypitch=100)), dict(d=desc(), sb=15),
           dict(d=desc(dst_offset=-4)), dict(d=desc(dst_offset=244)), dict(d=desc(), db=15), dict(d=nan), dict(d=inf),
           dict(d=desc(count=2, src_w=[4, 0]))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.ubd_last_error().decode().startswith("ubd_warp_images"), (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 9).all()                      # nothing was launched for a refused call
    # negative pitches are fine when the view stays inside the buffer
    assert call(desc(src_offset=15, src_xpitch=-1, src_ypitch=-4)) == 0
    torch.cuda.synchronize()
