"""GPU: the MEDIAN, HSV and ELASTIC modes of ubd_photometric_images (csrc/photometric.hip) and their place in the device
augmentation chain against the numpy oracle that defines them (tests/photometric_ext_oracle.py), np.array_equal throughout:
every mode on L / RGB images (HSV: RGB) from 1 x 1 up to two 64 x 16 tiles on both axes (the tile edge, one over, images smaller
than the halo), random pixels and 0 / 255 checkerboards, sources at +0 / +1 / +3 and destinations at +0 / +2 from a dword
boundary with guard bytes, every median size, the ends of the hue / saturation shifts and interior draws, in place, elastic
fields of both tap sets whose windows leave the image; a call that mixes old and new modes over more than one launch, graph
capture, every limit refused.  Then the chain: augment_arrays_on_device with plans sampled with photo_extended=True equals
Pillow's geometric chain followed by the oracles' stages."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import photometric_oracle as po  # noqa: E402
import photometric_ext_oracle as pe  # noqa: E402
from ubdvss_amd import NetConfig, ObjectMarkup, SegmapManager, _lib, synthetic  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

pytestmark = pytest.mark.gpu

# (w, h); the kernels' tile is 64 x 16: the edge, one over, two tiles on both axes, images smaller than the halo of 5
SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (11, 11), (63, 17), (64, 16), (65, 17), (130, 33)]
NEW = ("median_blur", "hue_saturation", "elastic")


def _f(mode, p, seed=0):
    return {"mode": mode, "flags": 0, "seed": int(seed), "p": [int(v) for v in p]}


def _params(mode, rng):
    if mode == pe.MEDIAN:
        return [_f(pe.MEDIAN, [k]) for k in (3, 5, 7, 9, 11)]
    if mode == pe.HSV:
        return [_f(pe.HSV, p) for p in ((0, 0), (-20, -20), (20, 20), (179, 255), (-179, -255), (255, -255),
                                        tuple(rng.integers(-20, 21, 2)), tuple(rng.integers(-255, 256, 2)))]
    seeds = [int(s) for s in rng.integers(0, 2 ** 64, 2, dtype=np.uint64)]
    return [_f(pe.ELASTIC, [aq, w0, w1], seed) for aq in (0, 128, 896, 4096) for w0, w1 in ((16374, 5), (8192, 4096)) for seed in seeds]


def _want(img, f):
    if f["mode"] >= pe.MEDIAN:
        return pe.apply(img, f["mode"], f["p"], f["flags"], f["seed"])
    return po.apply(img, f["mode"], f["p"], f["flags"], f["seed"])


def _call(lib, src_ptr, src_bytes, dst_ptr, dst_bytes, descs, c, stream=None):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    _lib.check(lib.ubd_photometric_images(src_ptr, src_bytes, dst_ptr, dst_bytes, descs.ctypes.data, c, len(descs), st),
               "ubd_photometric_images")


def _fill(d, f, w, h):
    d["w"], d["h"], d["mode"], d["flags"], d["seed"] = w, h, f["mode"], f["flags"], f["seed"]
    d["p"][:len(f["p"])] = f["p"]


def _device(jobs, c, misalign=(0, 1, 3), dst_misalign=(0, 2), in_place=False):
    """jobs: [(image, fields)].  All sources in one device buffer at +0 / +1 / +3 from a dword boundary, destinations at
    +0 / +2 with guard bytes between them, checked; the sources must come back unwritten; in_place: the destinations are the
    sources"""
    lib = _lib.load()
    offs, pos = [], 64
    for k, (a, _) in enumerate(jobs):
        pos = ((pos + 3) & ~3) + misalign[k % len(misalign)]
        offs.append(pos)
        pos += a.nbytes + (8 if in_place else 0)
    buf = np.full(pos + 64, 7, np.uint8)
    for (a, _), o in zip(jobs, offs):
        buf[o:o + a.nbytes] = a.reshape(-1)
    dbuf = torch.from_numpy(buf).cuda()
    if in_place:
        doffs, out = offs, dbuf
    else:
        doffs, pos = [], 16
        for k, (a, _) in enumerate(jobs):
            pos = ((pos + 3) & ~3) + dst_misalign[k % len(dst_misalign)]
            doffs.append(pos)
            pos += a.nbytes + 8
        out = torch.full((pos + 16,), 7, dtype=torch.uint8, device="cuda")
    descs = np.zeros(len(jobs), aug.PHOTO_DESC)
    for k, (a, f) in enumerate(jobs):
        descs[k]["src_offset"], descs[k]["dst_offset"] = offs[k], doffs[k]
        _fill(descs[k], f, a.shape[1], a.shape[0])
    _call(lib, dbuf.data_ptr(), dbuf.numel(), out.data_ptr(), out.numel(), descs, c)
    o = out.cpu().numpy()
    written = np.zeros(o.size, bool)
    res = []
    for (a, _), p in zip(jobs, doffs):
        res.append(o[p:p + a.nbytes].reshape(a.shape))
        written[p:p + a.nbytes] = True
    assert (o[~written] == 7).all(), "bytes outside the destinations were written"
    if not in_place:
        assert np.array_equal(dbuf.cpu().numpy(), buf), "the sources were written"
    return res


def _assert_jobs(jobs, got, tag):
    for k, ((a, f), g) in enumerate(zip(jobs, got)):
        want = _want(a, f)
        assert g.shape == want.shape and np.array_equal(g, want), (tag, k, a.shape, f, f"{int((g != want).sum())} bytes differ")


@pytest.mark.parametrize("mode,c", [(pe.MEDIAN, 1), (pe.MEDIAN, 3), (pe.HSV, 3), (pe.ELASTIC, 1), (pe.ELASTIC, 3)])
def test_mode_equals_the_oracle(mode, c):
    rng = np.random.default_rng(300 + 10 * mode + c)
    params = _params(mode, rng)
    jobs = []
    for si, (w, h) in enumerate(SIZES):
        for pi, f in enumerate(params):
            jobs.append((po.make_image(rng, h, w, c, checker=(si + pi) % 2 == 1), f))
    assert len(jobs) > 32                                                # more than one launch as well
    _assert_jobs(jobs, _device(jobs, c), (mode, c))
    if mode == pe.ELASTIC:                                               # aq = 0 is the identity; the other fields move pixels
        for a, f in jobs:
            if a.shape[:2] == (33, 130):
                assert np.array_equal(_want(a, f), a) == (f["p"][0] == 0)


def test_hsv_in_place():
    rng = np.random.default_rng(71)
    jobs = [(po.make_image(rng, h, w, 3, checker=False), f) for f in _params(pe.HSV, rng)[:4] for w, h in ((1, 1), (5, 3), (130, 33), (1025, 3))]
    _assert_jobs(jobs, _device(jobs, 3, in_place=True), "in place")


def test_elastic_of_a_constant_image():
    flat = np.full((60, 64, 3), 201, np.uint8)
    f = _f(pe.ELASTIC, [4096, 8192, 4096], 7)
    got = _device([(flat, f)], 3)[0]
    assert np.array_equal(got, _want(flat, f))
    assert (got[18:-18, 18:-18] == 201).all() and not (got == 201).all()  # constant wherever all 16 taps are inside


def _mixed_jobs(rng, c, n):
    modes = [po.AFFINE, pe.MEDIAN, po.BOX, pe.ELASTIC, po.DROPOUT, pe.HSV, po.SEP, po.FILTER3, po.GREY]
    St = aug.Stage
    old = {po.AFFINE: St("contrast", {"alphas": (1.7, 0.6, 1.2), "per_channel": True}, None), po.BOX: St("average_blur", {"k": 5}, None),
           po.DROPOUT: St("dropout", {"p": 0.05, "per_channel": True, "seed": 11}, None), po.SEP: St("gaussian_blur", {"sigma": 1.4}, None),
           po.FILTER3: St("sharpen", {"alpha": 0.5, "lightness": 1.2}, None), po.GREY: St("grayscale", {"alpha": 0.6}, None)}
    first = [(130, 33), (64, 64), (97, 35), (150, 20), (33, 70), (90, 41), (1, 9), (70, 18), (5, 5)]
    jobs = []
    for k in range(n):
        mode = modes[k % len(modes)]
        if mode in old:
            f = aug.photometric_descs(old[mode], 8, 8, c)
        else:
            ps = _params(mode, rng)
            f = ps[int(rng.integers(0, len(ps)))]
        w, h = first[k] if k < len(first) else (int(rng.integers(1, 150)), int(rng.integers(1, 60)))
        jobs.append((po.make_image(rng, h, w, c), f))
    return jobs


def test_one_call_mixes_old_and_new_modes_over_several_launches():
    jobs = _mixed_jobs(np.random.default_rng(61), 3, 9 * 34)             # 34 images of every mode: two launches of each kernel
    assert {f["mode"] for _, f in jobs} == {0, 1, 2, 3, 4, 6, 16, 17, 18}
    _assert_jobs(jobs, _device(jobs, 3), "mixed")


def test_graph_capture_replays_the_same_bytes():
    lib = _lib.load()
    rng = np.random.default_rng(91)
    jobs = _mixed_jobs(rng, 3, 18)
    sizes = [a.nbytes for a, _ in jobs]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in sizes])]).astype(np.int64)
    buf = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for (a, _), o in zip(jobs, offs):
        buf[int(o):int(o) + a.nbytes] = torch.from_numpy(a.reshape(-1)).cuda()
    descs = np.zeros(len(jobs), aug.PHOTO_DESC)
    for k, (a, f) in enumerate(jobs):
        descs[k]["src_offset"] = descs[k]["dst_offset"] = offs[k]
        _fill(descs[k], f, a.shape[1], a.shape[0])
    direct = torch.zeros_like(buf)
    out = torch.zeros_like(buf)
    _call(lib, buf.data_ptr(), buf.numel(), direct.data_ptr(), direct.numel(), descs, 3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(lib, buf.data_ptr(), buf.numel(), out.data_ptr(), out.numel(), descs, 3)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(lib, buf.data_ptr(), buf.numel(), out.data_ptr(), out.numel(), descs, 3)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)
    got = out.cpu().numpy()
    _assert_jobs(jobs, [got[int(offs[k]):int(offs[k]) + a.nbytes].reshape(a.shape) for k, (a, _) in enumerate(jobs)], "graph")


def test_limits_are_refused_with_a_message():
    lib = _lib.load()
    src = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    dst = torch.full((1024,), 9, dtype=torch.uint8, device="cuda")

    def desc(mode, p, **kw):
        d = np.zeros(1, aug.PHOTO_DESC)
        d["w"], d["h"], d["mode"] = 8, 8, mode
        d["p"][:, :len(p)] = p
        for k, v in kw.items():
            d[k] = v
        return d

    def call(d, c=3, s=None, t=None, sb=1024, db=1024):
        return lib.ubd_photometric_images(src.data_ptr() if s is None else s, sb, dst.data_ptr() if t is None else t, db,
                                          d.ctypes.data, c, len(d), None)
    good = [dict(d=desc(pe.MEDIAN, [3])), dict(d=desc(pe.MEDIAN, [11]), c=1), dict(d=desc(pe.HSV, [255, -255])), dict(d=desc(pe.HSV, [-255, 255])),
            dict(d=desc(pe.HSV, [0, 0]), s=dst.data_ptr()),                                  # in place: the same range
            dict(d=desc(pe.ELASTIC, [0, 16384, 0])), dict(d=desc(pe.ELASTIC, [4096, 0, 8192]), c=1), dict(d=desc(pe.ELASTIC, [896, 16374, 5])),
            dict(d=desc(pe.MEDIAN, [5]), s=dst.data_ptr(), sb=512, t=dst.data_ptr() + 512, db=512)]   # disjoint ranges of one buffer
    for kw in good:
        assert call(**kw) == 0, (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    dst.fill_(9)
    torch.cuda.synchronize()
    bad = [dict(d=desc(m, [3])) for m in (7, 8, 15, 19, 20, 32, -1)]
    bad += [dict(d=desc(pe.MEDIAN, [k])) for k in (0, 1, 2, 4, 10, 12, 13, -3)]
    bad += [dict(d=desc(pe.HSV, [0, 0]), c=1), dict(d=desc(pe.HSV, [256, 0])), dict(d=desc(pe.HSV, [-256, 0])), dict(d=desc(pe.HSV, [0, 256])),
            dict(d=desc(pe.HSV, [0, -256]))]
    bad += [dict(d=desc(pe.ELASTIC, p)) for p in ([-1, 16384, 0], [4097, 16384, 0], [128, 16386, -1], [128, -2, 8193], [128, 16384, 1],
                                                  [128, 16374, 4], [128, 0, 0])]
    # overlaps: the neighbourhood modes refuse every one, HSV all but the same range
    bad += [dict(d=desc(pe.MEDIAN, [3]), s=dst.data_ptr()), dict(d=desc(pe.ELASTIC, [128, 16374, 5]), s=dst.data_ptr()),
            dict(d=desc(pe.MEDIAN, [3]), s=dst.data_ptr(), sb=512, t=dst.data_ptr() + 191, db=512),
            dict(d=desc(pe.ELASTIC, [128, 16374, 5], dst_offset=32), s=dst.data_ptr()),
            dict(d=desc(pe.HSV, [1, 1], dst_offset=3), s=dst.data_ptr())]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.ubd_last_error().decode().startswith("ubd_photometric_images"), (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 9).all()                                # nothing was launched for a refused call
    assert lib.ubd_abi_version() == 3


# ---------------------------------------------------------------------------------------------------------------- the chain
def _pillow_chain(im, plan):
    for st in plan.stages:
        if st.kind in ("rotate", "quarter"):
            im = im.rotate(st.params["angle"], Image.BILINEAR, expand=True)
        elif st.kind == "crop":
            im = im.crop(st.params["box"])
        else:
            im = im.transform(im.size, Image.PERSPECTIVE, st.params["coeffs"], Image.BILINEAR)
    return im


def _pil(a):
    return Image.fromarray(a[..., 0] if a.shape[2] == 1 else a, "L" if a.shape[2] == 1 else "RGB")


def _arr(im):
    r = np.asarray(im)
    return r[..., None] if r.ndim == 2 else r


def _live_new(plan, c=3):
    """the new kinds of a plan that launch something"""
    return {st.kind for st in plan.photometric if st.kind in NEW and aug.photometric_descs(st, 8, 8, c) is not None}


def _chain_cases():
    """seeded (image, plan) pairs whose photometric plans hold each new kind at least twice, in different slots; plans with a
    NOISE stage (fp32 transcendentals: it would need the margin rule of tests/test_gpu_photometric.py) are passed over"""
    size = (90, 70)
    mk = [ObjectMarkup([30, 25, 60, 25, 60, 45, 30, 45])]
    rs = np.random.default_rng(12)
    need = {(k, n) for k in NEW for n in range(2)}
    slots = {k: set() for k in NEW}
    out = []
    for seed in range(5000):
        if not need:
            break
        plan = aug.sample_plan(size, mk, random.Random(seed), np.random.RandomState(seed), np.random.default_rng(seed), photo_extended=True)
        if any(st.kind == "noise" for st in plan.photometric):
            continue
        add = set()
        for i, st in enumerate(plan.photometric):
            if st.kind in _live_new(plan) and i not in slots[st.kind] and (st.kind, len(slots[st.kind])) in need:
                add.add((st.kind, len(slots[st.kind])))
                slots[st.kind].add(i)
        if add:
            need -= add
            out.append((rs.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8), plan))
    assert not need, need
    return out


def _assert_chain(got, a, plan, tag):
    c = a.shape[2]
    ref = _arr(_pillow_chain(_pil(a), plan))
    for st in () if plan.original else plan.photometric:
        f = aug.photometric_descs(st, ref.shape[1], ref.shape[0], c)
        if f is not None:
            assert f["mode"] != po.NOISE
            ref = _want(ref, f)
    assert got.shape == ref.shape and np.array_equal(got, ref), (tag, plan, f"{int((got != ref).sum())} bytes differ")


def test_device_chain_equals_pillow_then_the_oracles():
    cases = _chain_cases()
    assert set().union(*(_live_new(p) for _, p in cases)) == set(NEW)
    got = aug.augment_arrays_on_device([a for a, _ in cases], [p for _, p in cases])
    for k, ((a, plan), g) in enumerate(zip(cases, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("rgb", k))
    # grey images (hue_saturation launches nothing), sources on the device, read in place and never written
    greys = [np.ascontiguousarray(a[:, :, 1:2]) for a, _ in cases]
    tensors = [torch.from_numpy(a).cuda() for a in greys]
    got = aug.augment_arrays_on_device(tensors, [p for _, p in cases])
    for k, (a, (_, plan), t, g) in enumerate(zip(greys, cases, tensors, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("grey", k))
        assert np.array_equal(t.cpu().numpy(), a)
    # a caller's RGB tensor whose first stage is the in-place-capable HSV: it goes to a new buffer
    a = cases[0][0]
    plan = aug.AugmentationPlan((90, 70), (), False, True, (aug.Stage("hue_saturation", {"value": 7, "entry": 8}, None),
                                                           aug.Stage("unbuilt", {"name": "MedianBlur", "entry": 0}, None),
                                                           aug.Stage("median_blur", {"k": 5, "entry": 0}, None)))
    t = torch.from_numpy(a).cuda()
    g = aug.augment_arrays_on_device([t], [plan])[0]
    assert np.array_equal(t.cpu().numpy(), a) and g.data_ptr() != t.data_ptr()
    _assert_chain(g.cpu().numpy(), a, plan, "owned")


def _batch_plans(frames, markups, seed, extended):
    g = np.random.default_rng(seed)
    r, n = random.Random(seed), np.random.RandomState(seed)
    return [aug.sample_plan((a.shape[1], a.shape[0]), m, r, n, g, extended) for a, m in zip(frames, markups)]


def test_prepare_batches_with_the_extended_stage():
    cfg = NetConfig(grey=False)
    rs = np.random.default_rng(18)
    frames, markups = [], []
    for k in range(8):
        h, w = int(rs.integers(120, 200)), int(rs.integers(120, 200))
        frames.append(rs.integers(0, 256, (h, w, 3), dtype=np.uint8))
        markups.append([ObjectMarkup(q.reshape(-1).tolist()) for q in synthetic.random_quads(rs, h, w, 1, 3, 12, 40)])
    # one generator serves the whole batch, so an extended draw moves the stream of the images after it: the seed (found on the
    # CPU) is one where every image without a new stage still gets the plan of the default run
    for seed in range(2000):
        ext, plain = _batch_plans(frames, markups, seed, True), _batch_plans(frames, markups, seed, False)
        new = [bool(_live_new(p)) and not p.original for p in ext]
        if sum(new) >= 2 and all(n or e == p for n, e, p in zip(new, ext, plain)) and not any(st.kind == "noise" for p in ext for st in p.photometric):
            break
    else:
        raise AssertionError("no seed found")

    def run(extended):
        random.seed(seed)
        np.random.seed(seed)
        groups = SegmapManager.prepare_batches_on_device(frames, markups, cfg, augment=True, photo_rng=np.random.default_rng(seed),
                                                         photo_extended=extended)
        plans = {i: p for idx, _, _, _, ps in groups for i, p in zip(idx, ps)}
        images = {i: x.cpu().numpy()[j] for idx, x, _, _, _ in groups for j, i in enumerate(idx)}
        return [plans[i] for i in range(len(frames))], [images[i] for i in range(len(frames))]
    plans_e, img_e = run(True)
    plans_p, img_p = run(False)
    assert plans_e == ext and plans_p == plain
    for k, n in enumerate(new):
        assert img_e[k].shape == img_p[k].shape
        assert np.array_equal(img_e[k], img_p[k]) != n, (k, ext[k])
    # the extended images are the oracles' stages on Pillow's chain, rescaled like the others
    warped = aug.augment_arrays_on_device(frames, ext)
    for k, n in enumerate(new):
        if n:
            _assert_chain(warped[k].cpu().numpy(), frames[k], ext[k], ("batch", k))
            im, _ = SegmapManager._rescale_image_and_markup(_pil(warped[k].cpu().numpy()), aug.apply_plan_to_markup(ext[k], markups[k]), cfg)
            assert np.array_equal(img_e[k], _arr(im))
