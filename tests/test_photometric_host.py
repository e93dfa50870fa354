"""CPU: the host half of the photometric augmentation (ubdvss_amd/augmentation.py: sample_photometric, sample_plan's
photo_rng, photometric_descs) and the numpy oracle that defines the device modes (tests/photometric_oracle.py): Philox known
answers, the sampler's draws and ranges, the untouched geometric streams, every integer mode within one grey level of its
float64 formula (scipy.ndimage for the filters), the descriptor integers at the parameter extremes, and the share of NOISE
pixels the GPU test may excuse, from the oracle alone."""
import math
import os
import random
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import photometric_oracle as po  # noqa: E402
import ubdvss_amd  # noqa: E402
from ubdvss_amd import ObjectMarkup, _lib  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

SIDES = (1, 2, 3, 7, 40)
BUILT = {"gaussian_blur", "average_blur", "sharpen", "emboss", "noise", "dropout", "invert", "add", "multiply", "contrast", "grayscale"}


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = po.philox4x32_10(np.array([ctr], dtype=np.uint64), key)[0]
        assert tuple(int(v) for v in got) == want, (ctr, key, [hex(int(v)) for v in got])
    # the per-pixel words: counter (y w + x, 0, j, 0), key (seed lo, seed hi)
    r = po.pixel_words(2, 3, 0x299f31d0a4093822)
    assert r.shape == (2, 3, 8)
    for j in (0, 1):
        want = po.philox4x32_10(np.array([[5, 0, j, 0]], dtype=np.uint64), (0xa4093822, 0x299f31d0))[0]
        assert np.array_equal(r[1, 2, 4 * j:4 * j + 4], want)


def test_sampler_draws_and_ranges():
    assert ubdvss_amd.sample_photometric is aug.sample_photometric
    counts, kinds, unbuilt = set(), set(), set()
    for seed in range(2000):
        c = 1 if seed % 3 == 0 else 3
        stages = aug.sample_photometric(c, np.random.default_rng(seed))
        assert stages == aug.sample_photometric(c, np.random.default_rng(seed))
        assert isinstance(stages, tuple) and 0 <= len(stages) <= 5
        counts.add(len(stages))
        entries = [st.params["entry"] for st in stages]
        assert len(set(entries)) == len(entries) and all(0 <= e < 13 for e in entries)
        for st in stages:
            assert isinstance(st, aug.Stage) and st.size is None
            q = st.params
            kinds.add(st.kind)
            if st.kind == "unbuilt":
                unbuilt.add(q["name"])
                assert aug.photometric_descs(st, 9, 9, c) is None
            elif st.kind == "gaussian_blur":
                assert 0.0 <= q["sigma"] <= 3.0
            elif st.kind == "average_blur":
                assert q["k"] in range(2, 8)
            elif st.kind == "sharpen":
                assert 0.0 <= q["alpha"] <= 1.0 and 0.75 <= q["lightness"] <= 1.5
            elif st.kind == "emboss":
                assert 0.0 <= q["alpha"] <= 1.0 and 0.0 <= q["strength"] <= 2.0
            elif st.kind == "noise":
                assert 0.0 <= q["scale"] <= 0.05 * 255 and isinstance(q["per_channel"], bool) and 0 <= q["seed"] < 2 ** 64
            elif st.kind == "dropout":
                assert 0.01 <= q["p"] <= 0.1 and isinstance(q["per_channel"], bool) and 0 <= q["seed"] < 2 ** 64
            elif st.kind == "invert":
                assert len(q["channels"]) == c and all(isinstance(v, bool) for v in q["channels"])
            elif st.kind == "add":
                assert len(q["values"]) == c and all(isinstance(v, int) and -10 <= v <= 10 for v in q["values"])
                assert q["per_channel"] or len(set(q["values"])) == 1
            elif st.kind == "multiply":
                assert len(q["factors"]) == c and all(0.5 <= v <= 1.5 for v in q["factors"])
                assert q["per_channel"] or len(set(q["factors"])) == 1
            elif st.kind == "contrast":
                assert len(q["alphas"]) == c and all(0.5 <= v <= 2.0 for v in q["alphas"])
                assert q["per_channel"] or len(set(q["alphas"])) == 1
            else:
                assert st.kind == "grayscale" and 0.0 <= q["alpha"] <= 1.0
    assert counts == set(range(6))
    assert kinds == BUILT | {"unbuilt"}
    assert unbuilt == set(aug.PHOTO_UNBUILT) == {"MedianBlur", "SimplexNoiseAlpha", "AddToHueAndSaturation", "FrequencyNoiseAlpha",
                                                  "ElasticTransformation"}


def test_sampler_draw_order():
    """the first draws are the count and the permutation, then the entries' own draws in order"""
    for seed in range(50):
        g = np.random.default_rng(seed)
        n = int(g.integers(0, 6))
        order = g.permutation(13)[:n].tolist()
        stages = aug.sample_photometric(3, np.random.default_rng(seed))
        assert [st.params["entry"] for st in stages] == order
        if n and aug.PHOTO_ENTRIES[order[0]] == "sharpen":
            assert stages[0].params["alpha"] == float(g.uniform(0.0, 1.0)) and stages[0].params["lightness"] == float(g.uniform(0.75, 1.5))
        if n and aug.PHOTO_ENTRIES[order[0]] == "noise":
            assert stages[0].params["scale"] == float(g.uniform(0.0, 0.05 * 255))
            assert stages[0].params["per_channel"] == bool(g.random() < 0.5)
            assert stages[0].params["seed"] == int(g.integers(0, 2 ** 64, dtype=np.uint64))
        if n and aug.PHOTO_ENTRIES[order[0]] == "blur":
            assert {0: "gaussian_blur", 1: "average_blur", 2: "unbuilt"}[int(g.integers(0, 3))] == stages[0].kind


class _Log:
    """a generator proxy that logs every call and its result"""

    def __init__(self, gen):
        self._gen, self.log = gen, []

    def __getattr__(self, name):
        fn = getattr(self._gen, name)

        def call(*a):
            v = fn(*a)
            self.log.append((name, np.asarray(v).tolist()))
            return v
        return call


def test_sample_plan_keeps_the_geometric_streams():
    mk = [ObjectMarkup([100, 100, 200, 100, 200, 180, 100, 180])]
    filled = requested = 0
    for seed in range(300):
        r0, n0 = _Log(random.Random(seed)), _Log(np.random.RandomState(seed))
        plain = aug.sample_plan((640, 480), mk, r0, n0)
        r1, n1 = _Log(random.Random(seed)), _Log(np.random.RandomState(seed))
        photo = aug.sample_plan((640, 480), mk, r1, n1, np.random.default_rng(seed))
        assert r0.log == r1.log and n0.log == n1.log
        assert plain.photometric == () and plain[:4] == photo[:4]
        assert plain == aug.AugmentationPlan(plain.size, plain.stages, plain.original, plain.photometric_requested)   # four arguments
        if not photo.photometric_requested or photo.original:
            assert photo.photometric == () and photo == plain
        else:
            assert photo.photometric == aug.sample_photometric(3, np.random.default_rng(seed))
            requested += 1
            filled += bool(photo.photometric)
    assert requested > 150 and filled > 100
    # empty markup: nothing drawn from any generator
    g = np.random.default_rng(1)
    state = g.bit_generator.state
    for empty in ([], None):
        assert aug.sample_plan((640, 480), empty, random.Random(1), np.random.RandomState(1), g) == aug.AugmentationPlan((640, 480), (), False, False)
    assert g.bit_generator.state == state
    assert aug.identity_plan((3, 4)).photometric == ()


def _images():
    rng = np.random.default_rng(3)
    for h in SIDES:
        for w in SIDES:
            for c in (1, 3):
                yield po.make_image(rng, h, w, c, checker=False)
                yield po.make_image(rng, h, w, c, checker=True)


def _close(got, exact, tag):
    err = np.abs(got.astype(np.float64) - np.clip(exact, 0.0, 255.0))
    assert err.max() <= 1.0, (tag, got.shape, float(err.max()))


def test_pointwise_oracles_are_within_one_level_of_the_float_formula():
    rng = np.random.default_rng(4)
    for img in _images():
        c = img.shape[2]
        v = img.astype(np.float64)
        for _ in range(3):
            f, alpha, add = rng.uniform(0.5, 1.5, c), rng.uniform(0.5, 2.0, c), rng.integers(-10, 11, c)
            _close(po.affine(img, np.rint(f * 65536).astype(np.int64), [0] * c), f * v, "multiply")
            _close(po.affine(img, [65536] * c, add * 65536), v + add, "add")
            _close(po.affine(img, np.rint(alpha * 65536).astype(np.int64), np.rint(128 * (1 - alpha) * 65536).astype(np.int64)),
                   128 + alpha * (v - 128), "contrast")
            assert np.array_equal(po.affine(img, [-65536] * c, [255 * 65536] * c), 255 - img)
            a = float(rng.uniform(0, 1))
            if c == 3:
                g = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[..., None]
                _close(po.grey(img, int(np.rint(a * 16384))), (1 - a) * v + a * g, "grey")
            else:
                assert np.array_equal(po.grey(img, int(np.rint(a * 16384))), img)
        assert np.array_equal(po.grey(img, 0), img)


def test_filter_oracles_are_within_one_level_of_scipy():
    rng = np.random.default_rng(5)
    for img in _images():
        v = img.astype(np.float64)
        for kind in ("sharpen", "emboss"):
            alpha = float(rng.uniform(0, 1))
            params = {"alpha": alpha, "lightness": float(rng.uniform(0.75, 1.5)), "strength": float(rng.uniform(0, 2)), "entry": 1}
            l, s = params["lightness"], params["strength"]
            e = [[-1, -1, -1], [-1, 8 + l, -1], [-1, -1, -1]] if kind == "sharpen" else [[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]]
            k = (1 - alpha) * np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64) + alpha * np.array(e, np.float64)
            taps = aug.photometric_descs(aug.Stage(kind, params, None), img.shape[1], img.shape[0], img.shape[2])["p"]
            assert taps == np.rint(k * 16384).astype(np.int64).reshape(-1).tolist()
            exact = ndimage.correlate(v, k[:, :, None], mode="mirror")
            _close(po.filter3(img, taps), exact, kind)
        for sigma in (0.3, float(rng.uniform(0.2, 3.0)), 3.0):
            r, wts = aug.gaussian_taps(sigma)
            x = np.arange(-r, r + 1, dtype=np.float64)
            g = np.exp(-x * x / (2 * sigma * sigma))
            g /= g.sum()
            exact = ndimage.correlate1d(ndimage.correlate1d(v, g, axis=1, mode="mirror"), g, axis=0, mode="mirror")
            _close(po.sep(img, r, wts), exact, ("sep", sigma))
        for k in range(2, 8):
            # scipy centres a window of k at k // 2 with origin 0: offsets -(k // 2) .. k - 1 - k // 2, the anchor of the definition
            exact = ndimage.correlate(v, np.full((k, k, 1), 1.0 / (k * k)), mode="mirror", origin=0)
            _close(po.box(img, k), exact, ("box", k))


def test_reflect101():
    assert po.reflect101(np.arange(-7, 8), 1).tolist() == [0] * 15
    assert po.reflect101(np.arange(-5, 8), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert po.reflect101(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]


def _desc(kind, **params):
    return aug.photometric_descs(aug.Stage(kind, dict(params, entry=0), None), 10, 10, 3)


def test_descriptors_at_the_parameter_extremes():
    one = 16384
    assert _desc("sharpen", alpha=0.0, lightness=0.75) == {"mode": po.FILTER3, "flags": 0, "seed": 0, "p": [0, 0, 0, 0, one, 0, 0, 0, 0]}
    assert _desc("sharpen", alpha=1.0, lightness=1.5)["p"] == [-one] * 4 + [155648] + [-one] * 4
    assert _desc("emboss", alpha=0.0, strength=2.0)["p"] == [0, 0, 0, 0, one, 0, 0, 0, 0]
    assert _desc("emboss", alpha=1.0, strength=2.0)["p"] == [-3 * one, -2 * one, 0, -2 * one, one, 2 * one, 0, 2 * one, 3 * one]
    assert _desc("emboss", alpha=1.0, strength=0.0)["p"] == [-one, 0, 0, 0, one, 0, 0, 0, one]
    assert _desc("grayscale", alpha=0.0) == {"mode": po.GREY, "flags": 0, "seed": 0, "p": [0]}
    assert _desc("grayscale", alpha=1.0)["p"] == [one]
    assert aug.photometric_descs(aug.Stage("grayscale", {"alpha": 0.5}, None), 10, 10, 1) is None
    assert _desc("gaussian_blur", sigma=0.5e-3) is None
    d = _desc("gaussian_blur", sigma=1e-3)
    assert d["mode"] == po.SEP and d["p"] == [2, one, 0, 0]
    assert _desc("gaussian_blur", sigma=0.5)["p"] == [2, 12888, 1744, 4]
    for sigma in (1e-3, 0.5, 1.0, 1.6, 2.0, 2.5, 3.0):
        p = _desc("gaussian_blur", sigma=sigma)["p"]
        k = max(5, int(3.3 * sigma))
        assert p[0] == (k + 1 - k % 2) // 2 and 2 <= p[0] <= 4 and len(p) == p[0] + 2
        assert p[1] + 2 * sum(p[2:]) == one and all(0 <= v <= one for v in p[1:]) and p[1:] == sorted(p[1:], reverse=True)
    assert _desc("gaussian_blur", sigma=3.0)["p"][0] == 4
    assert _desc("average_blur", k=2) == {"mode": po.BOX, "flags": 0, "seed": 0, "p": [2]}
    assert _desc("average_blur", k=7)["p"] == [7]
    d = _desc("dropout", p=0.01, per_channel=False, seed=5)
    assert d == {"mode": po.DROPOUT, "flags": 0, "seed": 5, "p": [42949672]}
    d = _desc("dropout", p=0.1, per_channel=True, seed=2 ** 64 - 1)
    assert d == {"mode": po.DROPOUT, "flags": 1, "seed": 2 ** 64 - 1, "p": [429496729]}
    assert _desc("dropout", p=0.75, per_channel=False, seed=0)["p"] == [3 * 2 ** 30 - 2 ** 32]          # the uint32 bits in an int32
    assert _desc("noise", scale=0.0, per_channel=False, seed=1) == {"mode": po.NOISE, "flags": 0, "seed": 1, "p": [0]}
    assert _desc("noise", scale=12.75, per_channel=True, seed=1) == {"mode": po.NOISE, "flags": 1, "seed": 1, "p": [0x414C0000]}
    assert _desc("invert", channels=(True, False, True)) == {"mode": po.AFFINE, "flags": 0, "seed": 0,
                                                              "p": [-65536, 65536, -65536, 255 * 65536, 0, 255 * 65536]}
    assert _desc("add", values=(-10, 10, 0), per_channel=True)["p"] == [65536] * 3 + [-655360, 655360, 0]
    assert _desc("multiply", factors=(0.5, 1.5, 1.0), per_channel=True)["p"] == [32768, 98304, 65536, 0, 0, 0]
    assert _desc("contrast", alphas=(0.5, 2.0, 1.0), per_channel=True)["p"] == [32768, 131072, 65536, 4194304, -8388608, 0]
    grey = aug.photometric_descs(aug.Stage("contrast", {"alphas": (0.5, 2.0, 1.0), "per_channel": True}, None), 10, 10, 1)
    assert grey["p"] == [32768, 65536, 65536, 4194304, 0, 0]                                             # one channel: the first value
    assert aug.PHOTO_DESC.itemsize == 136 and aug.PHOTO_DESC.fields["seed"][1] == 32 and aug.PHOTO_DESC.fields["p"][1] == 40
    assert (_lib.UBD_PHOTO_AFFINE, _lib.UBD_PHOTO_DROPOUT) == (po.AFFINE, po.DROPOUT) == (0, 6)


def test_oracle_apply_follows_the_descriptor_layout():
    rng = np.random.default_rng(8)
    img = po.make_image(rng, 7, 9, 3, checker=False)
    d = _desc("gaussian_blur", sigma=1.3)
    assert np.array_equal(po.apply(img, d["mode"], d["p"]), po.sep(img, d["p"][0], d["p"][1:]))
    assert np.array_equal(po.apply(img, po.SEP, _desc("gaussian_blur", sigma=1e-3)["p"]), img)           # one tap of 16384: the identity
    d = _desc("dropout", p=0.75, per_channel=True, seed=77)
    got = po.apply(img, d["mode"], d["p"], d["flags"], d["seed"])
    assert np.array_equal(got, po.dropout(img, 3 * 2 ** 30, 1, 77)) and 0.5 < (got == 0).mean() < 0.95
    d = _desc("noise", scale=0.0, per_channel=True, seed=3)
    assert np.array_equal(po.apply(img, d["mode"], d["p"], d["flags"], d["seed"]), img)


def test_noise_share_near_a_rounding_boundary_is_small():
    """what tests/test_gpu_photometric.py may excuse, from the oracle alone: the fractional parts are spread evenly, so about
    2e-4 (1 + scale) of the pixels lie within the margin of a half-integer -- far below the 1 % cap of the GPU test"""
    total = 0
    for img, scale, pc, seed in po.noise_cases():
        out, exact = po.noise(img, scale, pc, seed)
        share = float(po.noise_excused(exact, scale).mean())
        assert share <= 0.01, (img.shape, scale, pc, share)
        if scale == 0.0:
            assert share == 0.0 and np.array_equal(out, img)
        else:
            assert not np.array_equal(out, img)
            z = (exact - img) / scale
            if img.size > 1000:
                assert abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05                                 # a standard normal field
                if img.shape[2] == 3:
                    assert np.allclose(z[..., 0], z[..., 1], atol=1e-9) != bool(pc)
        total += 1
    assert total == 12
