"""GPU: ubd_photometric_images (csrc/photometric.hip) and the photometric half of the device augmentation chain against the
numpy oracle that defines them (tests/photometric_oracle.py), np.array_equal: every mode on L / RGB images from 1 x 1 up to a few
tiles (the kernel's tile is 64 x 16: sizes at the edge, one below and one above on both axes, and 200 x 70, which has tiles
whose halo of up to 4 lies inside the image: the dword fill with its per-row byte phase), random pixels and +-255
checkerboards, sources at +0 / +1 / +3 and destinations at +0 / +2 from a dword boundary with guard bytes, the parameter ends
and interior draws, all blur radii and box sizes; mixed calls, more images than a launch takes, in place, graph capture, every
limit refused.  NOISE (fp32 logf / cosf on the device) may differ from the float64 oracle only where the oracle's unrounded
value lies within 1e-4 (1 + scale) of a half-integer, by one level, on at most 1 % of the pixels.  Then the chain:
augment_arrays_on_device with plans sampled with a photo_rng equals Pillow's geometric chain followed by the oracle's stages."""
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
from ubdvss_amd import NetConfig, ObjectMarkup, SegmapManager, _lib, synthetic  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

pytestmark = pytest.mark.gpu

TW, TH = 64, 16                                                         # PH_TW, PH_TH of csrc/photometric.hip
SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (8, 9), (63, 17), (64, 64), (65, 33), (130, 67),
         (TW, TH - 1), (TW - 1, TH), (TW + 1, TH + 1),
         (200, 70)]                                                     # (w, h); the last has tiles whose widest halo (4) is inside the image
POINTWISE = (po.AFFINE, po.GREY, po.NOISE, po.DROPOUT)


def _stage(kind, **params):
    return aug.Stage(kind, dict(params, entry=0), None)


def _fields(kind, c=3, **params):
    return aug.photometric_descs(_stage(kind, **params), 8, 8, c)


def _params(mode, rng):
    """descriptor fields at both ends of every range and at interior draws"""
    u = rng.uniform
    if mode == po.AFFINE:
        return [_fields("invert", channels=(True, True, True)), _fields("invert", channels=(False, True, False)),
                _fields("add", values=(-10, -10, -10), per_channel=False), _fields("add", values=(10, -3, 0), per_channel=True),
                _fields("multiply", factors=(0.5, 0.5, 0.5), per_channel=False), _fields("multiply", factors=(1.5, 0.5, float(u(0.5, 1.5))), per_channel=True),
                _fields("contrast", alphas=(0.5, 0.5, 0.5), per_channel=False), _fields("contrast", alphas=(2.0, 2.0, 2.0), per_channel=False),
                _fields("contrast", alphas=(float(u(0.5, 2.0)), 2.0, 0.5), per_channel=True)]
    if mode == po.GREY:
        return [_fields("grayscale", alpha=a) for a in (0.0, 1.0, float(u(0, 1)))]
    if mode == po.FILTER3:
        return [_fields("sharpen", alpha=0.0, lightness=0.75), _fields("sharpen", alpha=1.0, lightness=1.5),
                _fields("sharpen", alpha=float(u(0, 1)), lightness=float(u(0.75, 1.5))),
                _fields("emboss", alpha=0.0, strength=0.0), _fields("emboss", alpha=1.0, strength=2.0),
                _fields("emboss", alpha=float(u(0, 1)), strength=float(u(0, 2)))]
    if mode == po.SEP:
        out = [_fields("gaussian_blur", sigma=s) for s in (1e-3, 0.5, 2.2, 3.0, float(u(0.1, 3.0)))]
        assert {f["p"][0] for f in out} == {2, 3, 4}
        return out
    if mode == po.BOX:
        return [_fields("average_blur", k=k) for k in range(2, 8)]
    if mode == po.DROPOUT:
        return [_fields("dropout", p=p, per_channel=pc, seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
                for p in (0.01, 0.1, float(u(0.01, 0.1))) for pc in (False, True)]
    raise ValueError(mode)


def _call(lib, src_ptr, src_bytes, dst_ptr, dst_bytes, descs, c, stream=None):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    _lib.check(lib.ubd_photometric_images(src_ptr, src_bytes, dst_ptr, dst_bytes, descs.ctypes.data, c, len(descs), st),
               "ubd_photometric_images")


def _fill(d, f, w, h):
    d["w"], d["h"], d["mode"], d["flags"], d["seed"] = w, h, f["mode"], f["flags"], f["seed"]
    d["p"][:len(f["p"])] = f["p"]


def _device(jobs, c, misalign=(0, 1, 3), dst_misalign=(0, 2), in_place=False):
    """jobs: [(image, fields)].  All sources in one device buffer at +0 / +1 / +3 from a dword boundary, destinations at
    +0 / +2 with guard bytes between them, checked; in_place: the destinations are the sources"""
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


def _assert_noise(got, img, scale, flags, seed, tag):
    """the margin rule: exact everywhere except where the oracle's unrounded value is within 1e-4 (1 + scale) of a half-integer;
    there one of the two neighbouring levels; at most 1 % of the pixels excused"""
    want, exact = po.noise(img, scale, flags & 1, seed)
    excused = po.noise_excused(exact, scale)
    print(f"noise {tag}: {int(excused.sum())} of {excused.size} pixels near a half, {int((got != want).sum())} differ")
    assert excused.mean() <= 0.01, (tag, float(excused.mean()))
    assert np.array_equal(got[~excused], want[~excused]), (tag, int((got[~excused] != want[~excused]).sum()))
    lo, hi = np.clip(np.floor(exact), 0, 255), np.clip(np.ceil(exact), 0, 255)
    assert ((got == lo) | (got == hi))[excused].all(), tag


def _assert_stage(got, img, f, tag):
    if f["mode"] == po.NOISE:
        _assert_noise(got, img, float(np.array(f["p"][:1], np.int32).view(np.float32)[0]), f["flags"], f["seed"], tag)
    else:
        want = po.apply(img, f["mode"], f["p"], f["flags"], f["seed"])
        assert got.shape == want.shape and np.array_equal(got, want), (tag, img.shape, f, f"{int((got != want).sum())} bytes differ")


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("mode", [po.AFFINE, po.GREY, po.FILTER3, po.SEP, po.BOX, po.DROPOUT])
def test_mode_equals_the_oracle(mode, c):
    rng = np.random.default_rng(100 + 10 * mode + c)
    params = _params(mode, rng)
    jobs = []
    for si, (w, h) in enumerate(SIZES):
        for pi, f in enumerate(params):
            jobs.append((po.make_image(rng, h, w, c, checker=(si + pi) % 2 == 1), f))
    assert len(jobs) > 32                                                # more than one launch as well
    got = _device(jobs, c)
    for k, ((a, f), g) in enumerate(zip(jobs, got)):
        _assert_stage(g, a, f, (mode, c, k))


def _mixed_jobs(rng, c, n):
    modes = [po.AFFINE, po.GREY, po.FILTER3, po.SEP, po.BOX, po.NOISE, po.DROPOUT]
    jobs = []
    for k in range(n):
        mode = modes[k % 7]
        if mode == po.NOISE:
            f = _fields("noise", scale=0.5, per_channel=bool(k % 2), seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
        else:
            ps = _params(mode, rng)
            f = ps[int(rng.integers(0, len(ps)))]
        w, h = (int(rng.integers(1, 150)), int(rng.integers(1, 60))) if k >= 7 else [(130, 67), (64, 64), (97, 35), (150, 20), (33, 70), (90, 41), (1, 9)][k]
        jobs.append((po.make_image(rng, h, w, c), f))
    return jobs


@pytest.mark.parametrize("c", [1, 3])
def test_one_call_mixes_all_modes_and_sizes(c):
    jobs = _mixed_jobs(np.random.default_rng(50 + c), c, 7)
    assert {f["mode"] for _, f in jobs} == set(range(7))
    for k, ((a, f), g) in enumerate(zip(jobs, _device(jobs, c))):
        _assert_stage(g, a, f, ("mixed", c, k))


def test_more_images_than_one_launch():
    jobs = _mixed_jobs(np.random.default_rng(60), 3, 75)                  # 43 pointwise, 32 neighbourhood images: 2 + 1 launches
    for k, ((a, f), g) in enumerate(zip(jobs, _device(jobs, 3))):
        _assert_stage(g, a, f, ("launches", k))


@pytest.mark.parametrize("c", [1, 3])
def test_pointwise_modes_in_place(c):
    rng = np.random.default_rng(70 + c)
    jobs = []
    for mode in (po.AFFINE, po.GREY, po.DROPOUT):
        for f in _params(mode, rng)[:3]:
            for w, h in ((1, 1), (5, 3), (130, 67), (1025, 3)):
                jobs.append((po.make_image(rng, h, w, c), f))
    jobs.append((po.make_image(rng, 30, 41, c), _fields("noise", scale=0.5, per_channel=True, seed=9)))
    for k, ((a, f), g) in enumerate(zip(jobs, _device(jobs, c, in_place=True))):
        _assert_stage(g, a, f, ("in place", c, k))


def test_noise_within_the_margin_of_the_float64_oracle():
    cases = po.noise_cases()
    assert len(cases) == 12
    for c in (3, 1):
        sel = [(img, s, pc, seed) for img, s, pc, seed in cases if img.shape[2] == c]
        jobs = [(img, _fields("noise", c, scale=s, per_channel=bool(pc), seed=seed)) for img, s, pc, seed in sel]
        for k, ((img, s, pc, seed), g) in enumerate(zip(sel, _device(jobs, c))):
            _assert_noise(g, img, s, pc, seed, (img.shape, s, pc))
            if s == 0.0:
                assert np.array_equal(g, img)
            else:
                assert not np.array_equal(g, img)


def test_dropout_share():
    rng = np.random.default_rng(80)
    n = 256 * 256
    for c, pc, p in ((3, False, 0.05), (3, True, 0.1), (1, False, 0.01)):
        img = rng.integers(1, 256, (256, 256, c), dtype=np.uint8)        # no zero pixels of its own
        f = _fields("dropout", c, p=p, per_channel=pc, seed=1234567890123456789 + c)
        got = _device([(img, f)], c)[0]
        _assert_stage(got, img, f, ("dropout", c, pc))
        zero = got == 0
        if not pc:
            assert (zero.all(axis=2) == zero.any(axis=2)).all()          # whole pixels
        cnt = n * c if pc else n
        share = zero.sum() / (n * c)
        assert abs(share - p) <= 4 * np.sqrt(p * (1 - p) / cnt), (c, pc, p, share)


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


BUILT = ("gaussian_blur", "average_blur", "sharpen", "emboss", "noise", "dropout", "invert", "add", "multiply", "contrast", "grayscale")


def _chain_cases():
    """seeded (image, plan) pairs whose photometric plans hold every built kind in every slot 0..4; NOISE only as the last
    stage that changes pixels"""
    size = (90, 70)
    mk = [ObjectMarkup([30, 25, 60, 25, 60, 45, 30, 45])]
    rs = np.random.default_rng(11)
    need = {(k, s) for k in BUILT for s in range(5)}
    out = []
    for seed in range(40000):
        if not need:
            break
        plan = aug.sample_plan(size, mk, random.Random(seed), np.random.RandomState(seed), np.random.default_rng(seed))
        live = [i for i, st in enumerate(plan.photometric) if aug.photometric_descs(st, 8, 8, 3) is not None]
        noise_at = [i for i, st in enumerate(plan.photometric) if st.kind == "noise"]
        if noise_at and noise_at[0] != live[-1]:
            continue
        have = {(st.kind, i) for i, st in enumerate(plan.photometric)} & need
        if have:
            need -= have
            out.append((rs.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8), plan))
    assert not need, need
    return out


def _assert_chain(got, a, plan, tag):
    c = a.shape[2]
    ref = _arr(_pillow_chain(_pil(a), plan))
    stages = [] if plan.original else [f for f in (aug.photometric_descs(st, ref.shape[1], ref.shape[0], c) for st in plan.photometric) if f]
    for i, f in enumerate(stages):
        if f["mode"] == po.NOISE:
            assert i == len(stages) - 1
            assert got.shape == ref.shape
            _assert_stage(got, ref, f, tag)
            return
        ref = po.apply(ref, f["mode"], f["p"], f["flags"], f["seed"])
    assert got.shape == ref.shape and np.array_equal(got, ref), (tag, plan, f"{int((got != ref).sum())} bytes differ")


def test_device_chain_equals_pillow_then_the_oracle():
    cases = _chain_cases()
    assert any(p.stages for _, p in cases) and any(not p.stages for _, p in cases)
    got = aug.augment_arrays_on_device([a for a, _ in cases], [p for _, p in cases])
    for k, ((a, plan), g) in enumerate(zip(cases, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("rgb", k))
    # grey images (per-channel parameters: the first; grayscale: no launch), sources on the device, read in place
    sub = cases[::3]
    greys = [np.ascontiguousarray(a[:, :, 1:2]) for a, _ in sub]
    tensors = [torch.from_numpy(a).cuda() for a in greys]
    got = aug.augment_arrays_on_device(tensors, [p for _, p in sub])
    for k, (a, (_, plan), t, g) in enumerate(zip(greys, sub, tensors, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("grey", k))
        assert np.array_equal(t.cpu().numpy(), a)                        # the caller's tensor is untouched


def test_callers_tensor_is_never_written():
    rng = np.random.default_rng(13)
    a = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    chains = [(_stage("add", values=(5, 5, 5), per_channel=False), _stage("invert", channels=(True, False, True))),
              (_stage("dropout", p=0.1, per_channel=True, seed=4), _stage("average_blur", k=3), _stage("contrast", alphas=(2.0, 2.0, 2.0), per_channel=False)),
              (_stage("unbuilt", name="MedianBlur"), _stage("grayscale", alpha=0.7)),
              (_stage("unbuilt", name="MedianBlur"),)]
    plans = [aug.AugmentationPlan((50, 40), (), False, True, ch) for ch in chains]
    plans.append(aug.AugmentationPlan((50, 40), (), True, False, chains[0]))      # 'original': the stages are not run
    tensors = [torch.from_numpy(a).cuda() for _ in plans]
    got = aug.augment_arrays_on_device(tensors, plans)
    for k, (t, plan, g) in enumerate(zip(tensors, plans, got)):
        assert np.array_equal(t.cpu().numpy(), a), k
        _assert_chain(g.cpu().numpy(), a, plan, ("owned", k))
        changes = not plan.original and any(aug.photometric_descs(st, 50, 40, 3) for st in plan.photometric)
        assert (g.data_ptr() != t.data_ptr()) == changes
    # the same plans on host arrays (staged by the module, so the pointwise stages run in place)
    got = aug.augment_arrays_on_device([a.copy() for _ in plans], plans)
    for k, (plan, g) in enumerate(zip(plans, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("staged", k))


@pytest.mark.parametrize("grey", [True, False])
def test_prepare_batches_with_a_photo_rng(grey):
    cfg = NetConfig() if grey else NetConfig(grey=False)
    rs = np.random.default_rng(17)
    frames, markups = [], []
    for k in range(10):
        h, w = int(rs.integers(150, 300)), int(rs.integers(150, 300))
        frames.append(rs.integers(0, 256, (h, w, 3), dtype=np.uint8))
        markups.append([ObjectMarkup(q.reshape(-1).tolist()) for q in synthetic.random_quads(rs, h, w, 1, 3, 12, 40)])
    random.seed(5)
    np.random.seed(5)
    groups = SegmapManager.prepare_batches_on_device(frames, markups, cfg, augment=True, photo_rng=np.random.default_rng(5))
    plans = {i: p for idx, _, _, _, ps in groups for i, p in zip(idx, ps)}
    random.seed(5)
    np.random.seed(5)
    g = np.random.default_rng(5)
    again = [aug.sample_plan((a.shape[1], a.shape[0]), m, photo_rng=g) for a, m in zip(frames, markups)]
    assert [plans[i] for i in range(len(frames))] == again
    assert sum(bool(p.photometric) for p in again) >= 3
    assert any(aug.photometric_descs(st, 8, 8, 3) for p in again for st in p.photometric)
    warped = aug.augment_arrays_on_device(frames, again)
    plain = aug.augment_arrays_on_device(frames, [p._replace(photometric=()) for p in again])
    assert any(not torch.equal(x, y) for x, y in zip(warped, plain))       # the stage changed pixels
    for idx, x, _, _, _ in groups:
        xs = x.cpu().numpy()
        for j, i in enumerate(idx):
            im = _pil(warped[i].cpu().numpy())
            im, _ = SegmapManager._rescale_image_and_markup(im, aug.apply_plan_to_markup(again[i], markups[i]), cfg)
            ref = _arr(im.convert("L") if grey else im)
            assert xs[j].shape == ref.shape and np.array_equal(xs[j], ref), (i, again[i])


# ------------------------------------------------------------------------------------------------- refusals, graph capture
def test_limits_are_refused_with_a_message():
    lib = _lib.load()
    src = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    dst = torch.full((1024,), 9, dtype=torch.uint8, device="cuda")

    def desc(count=1, **kw):
        d = np.zeros(count, aug.PHOTO_DESC)
        d["w"], d["h"], d["mode"] = 8, 8, po.AFFINE
        d["p"][:, :3] = 65536
        for k, v in kw.items():
            if k == "p":
                d["p"][:, :len(v)] = v
            else:
                d[k] = v
        return d

    def call(d, c=1, n=None, s=None, t=None, sb=1024, db=1024, null_descs=False):
        return lib.ubd_photometric_images(src.data_ptr() if s is None else s, sb, dst.data_ptr() if t is None else t, db,
                                          None if null_descs else d.ctypes.data, c, len(d) if n is None else n, None)
    sep_ok = [2, 16384 - 2 * 3000 - 2 * 100, 3000, 100]
    good = [dict(d=desc()), dict(d=desc(), c=3), dict(d=desc(mode=po.BOX, p=[2])), dict(d=desc(mode=po.BOX, p=[7])),
            dict(d=desc(mode=po.SEP, p=[1, 16384 - 2 * 3000, 3000])), dict(d=desc(mode=po.SEP, p=sep_ok)),
            dict(d=desc(mode=po.SEP, p=[4, 16384, 0, 0, 0, 0])), dict(d=desc(src_offset=960, dst_offset=960)),
            dict(d=desc(p=[2 ** 17, -2 ** 17, 65536, 2 ** 24, -2 ** 24])), dict(d=desc(mode=po.GREY, p=[16384]), c=3),
            dict(d=desc(mode=po.FILTER3, p=[13 * 16384] * 9)), dict(d=desc(mode=po.NOISE, p=[0])),
            dict(d=desc(), s=dst.data_ptr()),                              # in place: the same range
            dict(d=desc(), s=dst.data_ptr(), sb=512, t=dst.data_ptr() + 64, db=512)]     # disjoint ranges of one buffer
    for kw in good:
        assert call(**kw) == 0, (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    dst.fill_(9)
    torch.cuda.synchronize()
    bad = [dict(d=desc(), n=0), dict(d=desc(), n=-1), dict(d=desc(), c=2), dict(d=desc(), c=4), dict(d=desc(), c=0), dict(d=desc(), s=0),
           dict(d=desc(), t=0), dict(d=desc(), null_descs=True), dict(d=desc(mode=7)), dict(d=desc(mode=-1)),
           dict(d=desc(w=0)), dict(d=desc(h=0)), dict(d=desc(w=16385, h=1)), dict(d=desc(w=1, h=16385)), dict(d=desc(w=-8)),
           dict(d=desc(src_offset=-1)), dict(d=desc(src_offset=961)), dict(d=desc(), sb=63), dict(d=desc(src_offset=2 ** 40)),
           dict(d=desc(dst_offset=-4)), dict(d=desc(dst_offset=961)), dict(d=desc(), db=63), dict(d=desc(), c=3, db=191),
           dict(d=desc(mode=po.BOX, p=[1])), dict(d=desc(mode=po.BOX, p=[8])), dict(d=desc(mode=po.BOX, p=[0])),
           dict(d=desc(mode=po.SEP, p=[0, 16384])), dict(d=desc(mode=po.SEP, p=[5, 16384, 0, 0, 0, 0, 0])), dict(d=desc(mode=po.SEP, p=[-1, 16384])),
           # a neighbourhood mode whose source and destination overlap; a pointwise mode that overlaps without being in place
           dict(d=desc(mode=po.BOX, p=[3]), s=dst.data_ptr()), dict(d=desc(mode=po.FILTER3, p=[0, 0, 0, 0, 16384]), s=dst.data_ptr(), sb=512, t=dst.data_ptr() + 63, db=512),
           dict(d=desc(mode=po.SEP, p=sep_ok, dst_offset=32), s=dst.data_ptr()),
           dict(d=desc(dst_offset=1), s=dst.data_ptr()),
           dict(d=desc(count=2, w=[8, 0])),
           # the parameter ranges behind the int32 bounds
           dict(d=desc(p=[2 ** 17 + 1])), dict(d=desc(p=[65536, -2 ** 17 - 1])), dict(d=desc(p=[65536, 65536, 65536, 2 ** 24 + 1])),
           dict(d=desc(p=[65536, 65536, 65536, 0, 0, -2 ** 24 - 1])), dict(d=desc(mode=po.GREY, p=[-1]), c=3), dict(d=desc(mode=po.GREY, p=[16385]), c=3),
           dict(d=desc(mode=po.FILTER3, p=[13 * 16384 + 1])), dict(d=desc(mode=po.FILTER3, p=[0] * 8 + [-13 * 16384 - 1])),
           dict(d=desc(mode=po.SEP, p=[1, 16384, 1])), dict(d=desc(mode=po.SEP, p=[1, 16386, -1])), dict(d=desc(mode=po.SEP, p=[2, 16384 - 2 * 16385, 0, 16385])),
           dict(d=desc(mode=po.NOISE, p=[0x7F800000])), dict(d=desc(mode=po.NOISE, p=[0x7FC00000])),
           dict(d=desc(mode=po.NOISE, p=[int(np.array([-1.0], np.float32).view(np.int32)[0])]))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.ubd_last_error().decode().startswith("ubd_photometric_images"), (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 9).all()                                # nothing was launched for a refused call
    # a 16384-wide image is inside the limits
    big = torch.zeros(16384 * 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(16384 * 3 + 4, dtype=torch.uint8, device="cuda")
    d = desc(w=16384, h=3, mode=po.BOX, p=[2], dst_offset=1)
    assert lib.ubd_photometric_images(big.data_ptr(), big.numel(), out.data_ptr(), out.numel(), d.ctypes.data, 1, 1, None) == 0
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


def test_graph_capture_replays_the_same_bytes():
    lib = _lib.load()
    rng = np.random.default_rng(90)
    jobs = _mixed_jobs(rng, 3, 14)
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
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, direct)
    got = out.cpu().numpy()
    for k, (a, f) in enumerate(jobs):
        _assert_stage(got[int(offs[k]):int(offs[k]) + a.nbytes].reshape(a.shape), a, f, ("graph", k))
