"""CPU: the host half of the geometric augmentation (ubdvss_amd/augmentation.py; reference augmentation.py:50-85): the plan
sampler consumes the generators in the reference's order and covers every branch, every planned size is Pillow's, the markup
transforms are exact where they must be (quarter turns, crops) and invert the stage's own matrix elsewhere, the caller's
markup is not mutated, and nothing runs without a GPU."""
import ctypes
import logging
import random

import numpy as np
import pytest
from PIL import Image

from ubdvss_amd import ObjectMarkup, ClassifiedObjectMarkup, NetConfig, SegmapManager, _lib
from ubdvss_amd import augmentation as aug


class Counting:
    """a generator proxy that logs (method, value) of every draw"""

    def __init__(self, gen):
        self._gen, self.log = gen, []

    def _wrap(self, name, *a):
        v = getattr(self._gen, name)(*a)
        self.log.append((name, v))
        return v

    def random(self):
        return self._wrap("random")

    def uniform(self, a, b):
        return self._wrap("uniform", a, b)

    def choice(self, seq):
        return self._wrap("choice", seq)


def _markup(rng, w, h, classified=False):
    out = []
    for k in range(int(rng.integers(1, 4))):
        cx, cy = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h
        rx, ry = rng.uniform(0.05, 0.2) * w, rng.uniform(0.05, 0.2) * h
        box = [int(cx - rx), int(cy - ry), int(cx + rx), int(cy - ry) + 1, int(cx + rx) + 1, int(cy + ry), int(cx - rx) - 1, int(cy + ry) + 2]
        out.append(ClassifiedObjectMarkup(box, k % 3) if classified else ObjectMarkup(box))
    return out


def _sample(seed, size=None):
    rs = np.random.default_rng(seed)
    size = (int(rs.integers(60, 2000)), int(rs.integers(60, 2000))) if size is None else size
    mk = _markup(rs, *size, classified=bool(seed % 2))
    r, n = Counting(random.Random(seed)), Counting(np.random.RandomState(seed))
    return size, mk, aug.sample_plan(size, mk, r, n), r, n


def test_sampler_consumes_the_generators_in_the_reference_order_and_covers_every_branch():
    combos, originals, photo = set(), 0, set()
    for seed in range(400):
        size, mk, plan, r, n = _sample(seed)
        kinds = tuple(s.kind for s in plan.stages)
        names = [name for name, _ in r.log]
        assert r.log[0][0] == "random" and plan.original == (r.log[0][1] < 0.1)
        if plan.original:
            assert names == ["random"] and n.log == [] and plan.stages == ()
            originals += 1
            continue
        expected = ["random"]                                           # feed original
        expected += ["random"] + ["uniform"] * ("rotate" in kinds)      # rotate
        expected += ["random"] + ["uniform"] * (4 * ("crop" in kinds))  # crop: left, top, right, bottom
        expected += ["random", "random"]                                # the two flips, probability 0
        expected += ["random"] + ["choice", "uniform"] * ("quarter" in kinds)
        expected += ["random"]                                          # perspective (drawn from numpy)
        expected += ["random"]                                          # photometric
        assert names == expected, (seed, names, expected)
        assert len(n.log) == ("perspective" in kinds)
        # every decision draw against its probability, and the values that went into the plan
        it = iter(r.log[1:])
        for kind, p, extra in (("rotate", 0.5, 1), ("crop", 0.5, 4), (None, 0, 0), (None, 0, 0), ("quarter", 0.5, 2), ("perspective", 0.5, 0)):
            _, v = next(it)
            assert (v < p) == (kind in kinds), (seed, kind, v)
            drawn = [next(it)[1] for _ in range(extra if kind in kinds else 0)]
            st = next((s for s in plan.stages if s.kind == kind), None)
            if kind == "rotate" and st:
                assert st.params["angle"] == drawn[0] and -45 <= drawn[0] <= 45
            if kind == "quarter" and st:
                assert st.params["angle"] == drawn[0] == drawn[1] and drawn[0] in (90, -90, 180)
            if kind == "crop" and st:
                w, h = plan.stages[0].size if kinds[0] == "rotate" else plan.size
                assert st.params["box"] == (drawn[0], drawn[1], w - drawn[2], h - drawn[3])
        _, v = next(it)
        assert plan.photometric_requested == (v < 0.7)
        if "perspective" in kinds:
            assert n.log[0][0] == "uniform" and n.log[0][1].shape == (8,)
            assert list(n.log[0][1]) == [s for s in plan.stages if s.kind == "perspective"][0].params["coeffs"]
        assert kinds == tuple(k for k in ("rotate", "crop", "quarter", "perspective") if k in kinds)      # the chain's order
        combos.add(kinds)
        photo.add(plan.photometric_requested)
        assert aug.sample_plan(size, mk, random.Random(seed), np.random.RandomState(seed)) == plan      # same seed, same plan
        assert "rotate" in repr(plan) or "rotate" not in kinds                                          # printable
    assert len(combos) == 16 and originals > 10 and photo == {True, False}


def test_empty_markup_draws_nothing():
    for mk in ([], None):
        r, n = Counting(random.Random(1)), Counting(np.random.RandomState(1))
        plan = aug.sample_plan((640, 480), mk, r, n)
        assert plan == aug.AugmentationPlan((640, 480), (), False, False) and r.log == [] and n.log == []


def test_default_generators_are_the_modules():
    """seeding `random` and `numpy.random` as augmentation.py:29-31 invites gives the stream of explicit generators"""
    mk = [ObjectMarkup([100, 100, 300, 110, 310, 200, 90, 190])]
    for seed in range(20):
        random.seed(seed)
        np.random.seed(seed)
        assert aug.sample_plan((800, 600), mk) == aug.sample_plan((800, 600), mk, random.Random(seed), np.random.RandomState(seed))


def test_planned_sizes_are_pillows():
    n = {"rotate": 0, "crop": 0, "quarter": 0, "perspective": 0}
    for seed in range(300):
        size, _, plan, _, _ = _sample(seed)
        for st in plan.stages:
            im = Image.new("L", size)
            if st.kind in ("rotate", "quarter"):
                got = im.rotate(st.params["angle"], Image.BILINEAR, expand=True).size
            elif st.kind == "crop":
                got = im.crop(st.params["box"]).size
                assert aug.crop_window(st.params["box"]) == st.params["window"]
            else:
                got = size
            assert got == tuple(st.size), (seed, st, got)
            size = tuple(st.size)
            n[st.kind] += 1
    assert min(n.values()) > 50
    for angle in (0.0, 360.0, 90.0, -90.0, 180.0, 270.0, 1e-12, 44.99999, -45.0):       # Image.rotate's special cases
        for size in ((1, 1), (7, 3), (640, 480), (1, 900)):
            assert aug.rotate_matrix_and_size(angle, size)[2] == Image.new("L", size).rotate(angle, Image.BILINEAR, expand=True).size


def test_quarter_turns_of_integer_markup_are_exact_integers():
    rs = np.random.default_rng(0)
    for _ in range(200):
        w, h = int(rs.integers(1, 4000)), int(rs.integers(1, 4000))
        box = rs.integers(-50, 4100, 8).tolist()
        pts = np.array(box).reshape(4, 2)
        for angle, size, closed in ((90, (h, w), [(y, w - x) for x, y in pts]), (-90, (h, w), [(h - y, x) for x, y in pts]),
                                    (180, (w, h), [(w - x, h - y) for x, y in pts])):
            plan = aug.AugmentationPlan((w, h), (aug.Stage("quarter", {"angle": angle}, size),), False, False)
            got = aug.apply_plan_to_markup(plan, [ObjectMarkup(box)])[0].bbox
            assert got.dtype == np.float64 and (got == np.array(closed, np.float64).reshape(-1)).all(), (w, h, angle, got, closed)
    # and the pixel that a markup corner sits on goes where the image's pixel goes
    a = np.arange(6 * 4, dtype=np.uint8).reshape(4, 6)                                # h = 4, w = 6
    for angle in (90, -90, 180):
        im = Image.fromarray(a).rotate(angle, Image.BILINEAR, expand=True)
        plan = aug.AugmentationPlan((6, 4), (aug.Stage("quarter", {"angle": angle}, im.size),), False, False)
        # the pixel SQUARE [2, 3] x [1, 2] of value a[1, 2]: its centre (2.5, 1.5) moves with the markup
        cx, cy = aug.apply_plan_to_markup(plan, [ObjectMarkup([2.5, 1.5] * 4)])[0].bbox[:2]
        assert np.asarray(im)[int(cy), int(cx)] == a[1, 2]


def test_rotation_and_perspective_markup_invert_the_stage_matrix():
    n_rot = n_per = 0
    for seed in range(300):
        size, mk, plan, _, _ = _sample(seed)
        pts = [np.array(m.bbox, np.float64).reshape(-1, 2) for m in mk]
        for st in plan.stages:
            new = [aug._stage_points(st, p, size) for p in pts]
            if st.kind == "rotate":
                kind, m, _ = aug.rotate_matrix_and_size(st.params["angle"], size)
                assert kind == "affine"
                back = [np.stack([m[0] * q[:, 0] + m[1] * q[:, 1] + m[2], m[3] * q[:, 0] + m[4] * q[:, 1] + m[5]], 1) for q in new]
                n_rot += 1
            elif st.kind == "perspective":
                a = st.params["coeffs"]
                den = [a[6] * q[:, 0] + a[7] * q[:, 1] + 1 for q in new]
                back = [np.stack([(a[0] * q[:, 0] + a[1] * q[:, 1] + a[2]) / d, (a[3] * q[:, 0] + a[4] * q[:, 1] + a[5]) / d], 1)
                        for q, d in zip(new, den)]
                n_per += 1
            elif st.kind == "crop":
                left, top = st.params["box"][:2]
                for p, q in zip(pts, new):
                    assert (q[:, 0] == p[:, 0] + -left).all() and (q[:, 1] == p[:, 1] + -top).all()
                back = None
            else:
                back = None
            if back is not None:
                for p, b in zip(pts, back):
                    assert np.abs(p - b).max() < 1e-6, (seed, st, np.abs(p - b).max())
            pts, size = new, tuple(st.size)
        # the whole plan, through the public function: same numbers, same types, the caller's objects untouched
        before = [(type(m), list(m.bbox), getattr(m, "object_type", None)) for m in mk]
        ids = [id(m.bbox) for m in mk]
        out = aug.apply_plan_to_markup(plan, mk)
        assert [(type(m), list(m.bbox), getattr(m, "object_type", None)) for m in mk] == before and [id(m.bbox) for m in mk] == ids
        for m, o, p in zip(mk, out, pts):
            assert type(o) is type(m) and getattr(o, "object_type", None) == getattr(m, "object_type", None)
            assert o is not m and (np.asarray(o.bbox) == p.reshape(-1)).all()
    assert n_rot > 50 and n_per > 50


def test_degenerate_stages_are_skipped_with_a_warning(caplog):
    flat = [ObjectMarkup([10, 20, 50, 20, 50, 20, 10, 20])]                         # markup bounds without height
    seen = 0
    for seed in range(60):
        r = Counting(random.Random(seed))
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            plan = aug.sample_plan((200, 100), flat, r, Counting(np.random.RandomState(seed)))
        if plan.original:
            continue
        assert "crop" not in [s.kind for s in plan.stages] or "rotate" in [s.kind for s in plan.stages]   # a rotation gives it height
        names = [n for n, _ in r.log]
        wanted = r.log[2 + ("rotate" in [s.kind for s in plan.stages])][1] < 0.5   # the crop's decision draw
        if wanted and "rotate" not in [s.kind for s in plan.stages]:
            assert "crop skipped" in caplog.text
            assert names.count("uniform") == ("quarter" in [s.kind for s in plan.stages])   # no crop draws, the chain went on
            seen += 1
    assert seen > 5
    # a crop that rounds to an empty window on a tiny image
    tiny = [ObjectMarkup([0, 0, 2, 0, 2, 2, 0, 2])]
    kinds = set()
    for seed in range(200):
        plan = aug.sample_plan((2, 2), tiny, random.Random(seed), np.random.RandomState(seed))
        for st in plan.stages:
            assert st.size[0] >= 1 and st.size[1] >= 1
            kinds.add(st.kind)
    assert "crop" in kinds


def test_no_gpu_no_run():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    im = Image.new("RGB", (64, 48))
    mk = [ObjectMarkup([10, 10, 30, 10, 30, 30, 10, 30])]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug.SegLinksImageAugmentation(im, mk, NetConfig())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SegmapManager.prepare_image_and_target(im, mk, NetConfig(), augment=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SegmapManager.prepare_batches_on_device([im], [mk], NetConfig())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug.augment_arrays_on_device([np.zeros((4, 4, 3), np.uint8)], [aug.identity_plan((4, 4))])
    # augment=False is what it was: pure host code
    image, markup, seg = SegmapManager.prepare_image_and_target(im, mk, NetConfig(), augment=False)
    assert image.size == (64, 64) and seg.size == (16, 16)
    # the C entry point: a dummy pointer gets as far as the launch, which fails without a device
    lib = _lib.load()
    d = np.zeros(1, aug.WARP_DESC)
    d["src_xpitch"], d["src_ypitch"], d["src_w"], d["src_h"], d["dst_w"], d["dst_h"], d["mode"] = 1, 4, 4, 4, 4, 4, 1
    d["coeffs"][0, :6] = [1, 0, 0, 0, 1, 0]
    assert lib.ubd_warp_images(ctypes.c_void_p(4096), 16, ctypes.c_void_p(8192), 16, d.ctypes.data, 1, 1, None) != 0
    assert lib.ubd_last_error()
    assert lib.ubd_warp_images(ctypes.c_void_p(4096), 16, ctypes.c_void_p(8192), 16, d.ctypes.data, 2, 1, None) != 0
    assert lib.ubd_last_error().decode().startswith("ubd_warp_images")


def test_exports():
    import ubdvss_amd
    for name in ("SegLinksImageAugmentation", "AugmentationPlan", "Stage", "sample_plan", "apply_plan_to_markup"):
        assert hasattr(ubdvss_amd, name)
    assert "ubd_warp_images" in _lib.SIGNATURES
    assert aug.WARP_DESC.itemsize == 112
