"""CPU: the host half of the three extended photometric operations (MedianBlur, AddToHueAndSaturation, ElasticTransformation;
ubdvss_amd/augmentation.py: sample_photometric(extended=True), sample_plan(photo_extended=True), photometric_descs) and the numpy
oracle that defines their device modes (tests/photometric_ext_oracle.py): the default sampler is unchanged, the extended
sampler's draws and ranges, the untouched geometric streams, the median against scipy.ndimage, the integer HSV and the integer
bicubic gather within one level of their float64 formulas, the statistics of the displacement field, the descriptor integers.

The displacement field's expected deviation: the raw field is uniform in (-1, 1) (variance 1 / 3) and is smoothed on both axes
by the taps (w1, w0, w1) / 16384, so the deviation of s / 32768 is (w0^2 + 2 w1^2) / 16384^2 / sqrt(3)."""
import os
import random
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import photometric_oracle as po  # noqa: E402
import photometric_ext_oracle as pe  # noqa: E402
from ubdvss_amd import ObjectMarkup, _lib  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

SIDES = (1, 2, 3, 7, 40)
BUILT = {"gaussian_blur", "average_blur", "sharpen", "emboss", "noise", "dropout", "invert", "add", "multiply", "contrast", "grayscale"}
NEW = {"median_blur", "hue_saturation", "elastic"}


def test_default_sampler_is_unchanged():
    kinds = set()
    for seed in range(500):
        c = 1 if seed % 3 == 0 else 3
        plain = aug.sample_photometric(c, np.random.default_rng(seed))
        assert plain == aug.sample_photometric(c, np.random.default_rng(seed), extended=False)
        assert plain == aug.sample_photometric(c, np.random.default_rng(seed), False)
        kinds |= {st.kind for st in plain}
    assert kinds == BUILT | {"unbuilt"}
    assert aug.PHOTO_UNBUILT == ("MedianBlur", "SimplexNoiseAlpha", "AddToHueAndSaturation", "FrequencyNoiseAlpha", "ElasticTransformation")
    assert aug.PHOTO_EXTENDED == ("MedianBlur", "AddToHueAndSaturation", "ElasticTransformation")
    assert (_lib.UBD_PHOTO_MEDIAN, _lib.UBD_PHOTO_HSV, _lib.UBD_PHOTO_ELASTIC) == (pe.MEDIAN, pe.HSV, pe.ELASTIC) == (16, 17, 18)


def test_extended_sampler_draws_and_ranges():
    ks, values, unbuilt, kinds, applied = [], set(), set(), set(), set()
    for seed in range(3000):
        c = 1 if seed % 3 == 0 else 3
        g = np.random.default_rng(seed)
        n = int(g.integers(0, 6))
        order = g.permutation(13)[:n].tolist()
        stages = aug.sample_photometric(c, np.random.default_rng(seed), extended=True)
        assert stages == aug.sample_photometric(c, np.random.default_rng(seed), True)
        assert [st.params["entry"] for st in stages] == order              # the entry order is the permutation
        plain = aug.sample_photometric(c, np.random.default_rng(seed))
        assert [st.params["entry"] for st in plain] == order
        # every stage before the first extended entry comes from the same draws as in the default call
        first = next((i for i, st in enumerate(plain) if st.kind == "unbuilt" and st.params["name"] in aug.PHOTO_EXTENDED), len(plain))
        assert stages[:first] == plain[:first]
        if first < len(plain):
            assert stages[first].kind in NEW
        for st in stages:
            assert isinstance(st, aug.Stage) and st.size is None
            kinds.add(st.kind)
            q = st.params
            if st.kind == "unbuilt":
                unbuilt.add(q["name"])
                assert aug.photometric_descs(st, 9, 9, c) is None
            elif st.kind == "median_blur":
                assert set(q) == {"k", "entry"} and isinstance(q["k"], int)
                ks.append(q["k"])
            elif st.kind == "hue_saturation":
                assert set(q) == {"value", "entry"} and isinstance(q["value"], int)
                values.add(q["value"])
            elif st.kind == "elastic":
                applied.add(q["applied"])
                assert q["sigma"] == 0.25
                if q["applied"]:
                    assert set(q) == {"applied", "alpha", "sigma", "seed", "entry"}
                    assert 0.5 <= q["alpha"] <= 3.5 and isinstance(q["seed"], int) and 0 <= q["seed"] < 2 ** 64
                else:
                    assert set(q) == {"applied", "sigma", "entry"}
                    assert aug.photometric_descs(st, 9, 9, c) is None
    assert kinds == BUILT | NEW | {"unbuilt"}
    assert unbuilt == set(aug.PHOTO_UNBUILT) - set(aug.PHOTO_EXTENDED) == {"SimplexNoiseAlpha", "FrequencyNoiseAlpha"}
    count = {k: ks.count(k) for k in set(ks)}
    assert set(count) == {3, 5, 7, 9, 11}                                 # 4, 6, 8, 10 become the next odd size: 3 has half the share
    assert all(count[3] < count[k] for k in (5, 7, 9, 11)), count
    assert values == set(range(-20, 21))
    assert applied == {True, False}


def test_extended_draw_order_of_the_new_entries():
    seen = set()
    for seed in range(400):
        g = np.random.default_rng(seed)
        n = int(g.integers(0, 6))
        order = g.permutation(13)[:n].tolist()
        stages = aug.sample_photometric(3, np.random.default_rng(seed), extended=True)
        if not n:
            continue
        name, st = aug.PHOTO_ENTRIES[order[0]], stages[0]
        if name == "blur" and int(g.integers(0, 3)) == 2:
            k = int(g.integers(3, 12))
            assert st.kind == "median_blur" and st.params["k"] == (k + 1 if k % 2 == 0 else k)
            seen.add("median")
        elif name == "hue_saturation":
            assert st.kind == "hue_saturation" and st.params["value"] == int(g.integers(-20, 21))
            seen.add("hsv")
        elif name == "elastic":
            assert st.kind == "elastic" and st.params["applied"] == bool(g.random() < 0.5)
            if st.params["applied"]:
                assert st.params["alpha"] == float(g.uniform(0.5, 3.5))
                assert st.params["seed"] == int(g.integers(0, 2 ** 64, dtype=np.uint64))
                seen.add("elastic")
    assert seen == {"median", "hsv", "elastic"}


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


def test_sample_plan_extended_keeps_the_geometric_streams():
    mk = [ObjectMarkup([100, 100, 200, 100, 200, 180, 100, 180])]
    new = 0
    for seed in range(300):
        r0, n0 = _Log(random.Random(seed)), _Log(np.random.RandomState(seed))
        plain = aug.sample_plan((640, 480), mk, r0, n0, np.random.default_rng(seed))
        assert plain == aug.sample_plan((640, 480), mk, random.Random(seed), np.random.RandomState(seed), np.random.default_rng(seed), False)
        r1, n1 = _Log(random.Random(seed)), _Log(np.random.RandomState(seed))
        ext = aug.sample_plan((640, 480), mk, r1, n1, photo_rng=np.random.default_rng(seed), photo_extended=True)
        assert r0.log == r1.log and n0.log == n1.log
        assert plain[:4] == ext[:4]
        if ext.photometric_requested and not ext.original:
            assert ext.photometric == aug.sample_photometric(3, np.random.default_rng(seed), extended=True)
            new += any(st.kind in NEW for st in ext.photometric)
        else:
            assert ext.photometric == ()
        # without a generator the flag draws nothing
        assert aug.sample_plan((640, 480), mk, random.Random(seed), np.random.RandomState(seed), photo_extended=True).photometric == ()
    assert new > 30


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
def test_median_equals_scipy(k):
    rng = np.random.default_rng(20 + k)
    for h in SIDES:
        for w in SIDES:
            for c in (1, 3):
                for checker in (False, True):
                    img = po.make_image(rng, h, w, c, checker=checker)
                    want = ndimage.median_filter(img, size=(k, k, 1), mode="nearest")
                    assert np.array_equal(pe.median(img, k), want), (k, h, w, c, checker)
                    assert np.array_equal(pe.apply(img, pe.MEDIAN, [k]), want)


def _colours():
    rng = np.random.default_rng(30)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    prim = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]], np.uint8)
    return np.concatenate([rng.integers(0, 256, (20000, 3), dtype=np.uint8), grey, prim, prim // 2])[None]


def _hsv_float(img):
    v = img.astype(np.float64)
    R, G, B = v[..., 0], v[..., 1], v[..., 2]
    V = v.max(-1)
    D = V - v.min(-1)
    S = np.where(V > 0, 255.0 * D / np.maximum(V, 1), 0.0)
    hn = np.where(V == R, G - B, np.where(V == G, B - R + 2 * D, R - G + 4 * D))
    H = np.where(D > 0, 30.0 * hn / np.maximum(D, 1), 0.0)
    return np.where(H < 0, H + 180.0, H), S, V


def _rgb_float(H, S, V):
    H, S, V = (np.asarray(a, np.float64) for a in (H, S, V))
    i = np.floor(H / 30.0)
    f = H / 30.0 - i
    s = S / 255.0
    P, Q, T = V * (1 - s), V * (1 - s * f), V * (1 - s * (1 - f))
    table = ((V, T, P), (Q, V, P), (P, V, T), (P, Q, V), (T, P, V), (V, P, Q))
    return np.stack([np.select([i == k for k in range(6)], [table[k][ch] for k in range(6)]) for ch in range(3)], -1)


def test_hsv_against_float64():
    img = _colours()
    H, S, V = pe.hsv_forward(img)
    assert H.min() >= 0 and H.max() <= 179 and S.min() >= 0 and S.max() <= 255
    Hf, Sf, Vf = _hsv_float(img)
    dh = np.abs(H - Hf)
    assert np.minimum(dh, 180.0 - dh).max() <= 1.0 and np.abs(S - Sf).max() <= 1.0 and np.array_equal(V, Vf)
    for dhue, dsat in ((0, 0), (-20, -20), (20, 20), (77, -100), (-179, 255), (255, -255)):
        H2, S2 = np.mod(H + dhue, 180), np.clip(S + dsat, 0, 255)
        got = pe.hsv(img, dhue, dsat)
        assert np.abs(got.astype(np.float64) - _rgb_float(H2, S2, V)).max() <= 1.0           # backward within one level
        assert np.array_equal(got, pe.hsv_backward(H2, S2, V)) and np.array_equal(got, pe.apply(img, pe.HSV, [dhue, dsat]))
        assert np.array_equal(got.max(-1), V)                                               # V is preserved
    grey = pe.hsv(img, 0, -255)
    assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 1] == grey[..., 2]).all()     # S' = 0: fully grey
    sat = pe.hsv(img, 0, 255)
    assert (sat.min(-1) == 0).all()                                                         # S' = 255: P = 0
    assert np.array_equal(pe.hsv(img, 180, 5), pe.hsv(img, 0, 5)) and np.array_equal(pe.hsv(img, -180, 5), pe.hsv(img, 0, 5))
    with pytest.raises(ValueError):
        pe.hsv(img[..., :1], 0, 0)


def test_keys_weights_sum_to_one():
    wts = pe.keys_weights(np.arange(32))
    assert wts.shape == (32, 4) and (wts.sum(-1) == 131072).all()
    assert wts[0].tolist() == [0, 131072, 0, 0]
    assert np.array_equal(wts[1:], wts[1:][::-1, ::-1])                   # phase k mirrors phase 32 - k


def _keys(t, a=-0.75):
    t = np.abs(t)
    return np.where(t <= 1, (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1, np.where(t < 2, a * t ** 3 - 5 * a * t ** 2 + 8 * a * t - 4 * a, 0.0))


def _elastic_float(img, X, Y):
    h, w, c = img.shape
    fx, fy = X / 32.0, Y / 32.0
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    v = img.astype(np.float64)
    acc = np.zeros((h, w, c))
    for j in range(-1, 3):
        for i in range(-1, 3):
            xx, yy = ix + i, iy + j
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            tap = v[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]
            acc += (_keys(fx - xx) * _keys(fy - yy))[..., None] * tap
    return np.clip(acc, 0.0, 255.0)


def test_elastic_oracle():
    rng = np.random.default_rng(40)
    for h, w, c in ((1, 1, 1), (3, 4, 3), (7, 40, 1), (40, 37, 3)):
        img = po.make_image(rng, h, w, c, checker=False)
        for taps in ((16374, 5), (8192, 4096), (16384, 0)):
            for seed in (1, 2 ** 64 - 1):
                assert np.array_equal(pe.elastic(img, 0, *taps, seed), img)                  # aq = 0: the identity
        for aq in (128, 896, 4096):
            for taps in ((16374, 5), (8192, 4096)):
                seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
                got = pe.elastic(img, aq, *taps, seed)
                assert np.array_equal(got, pe.apply(img, pe.ELASTIC, [aq, *taps], 0, seed))
                X, Y = pe.elastic_positions(h, w, aq, *taps, seed)
                assert np.abs(X - 32 * np.arange(w)[None, :]).max() <= aq // 8 and np.abs(Y - 32 * np.arange(h)[:, None]).max() <= aq // 8
                assert np.abs(got.astype(np.float64) - _elastic_float(img, X, Y)).max() <= 1.0, (h, w, c, aq, taps)
    # a constant image stays constant wherever all 16 taps are inside: 16 pixels of displacement plus the 2 taps beyond
    flat = np.full((60, 64, 3), 201, np.uint8)
    got = pe.elastic(flat, 4096, 8192, 4096, 7)
    assert (got[18:-18, 18:-18] == 201).all() and not (got == 201).all()
    # two seeds give two fields
    img = po.make_image(rng, 30, 30, 3, checker=False)
    assert not np.array_equal(pe.elastic(img, 896, 16374, 5, 1), pe.elastic(img, 896, 16374, 5, 2))


@pytest.mark.parametrize("taps", [(16374, 5), (8192, 4096)])
def test_elastic_field_statistics(taps):
    w0, w1 = taps
    sx, sy = pe.elastic_field(200, 200, w0, w1, 0x123456789abcdef)
    want = (w0 * w0 + 2 * w1 * w1) / 16384.0 ** 2 / np.sqrt(3.0)
    for s in (sx, sy):
        f = s / 32768.0
        assert np.abs(f).max() <= 1.0
        assert abs(f.mean()) < 0.02, (taps, f.mean())
        assert abs(f.std() / want - 1.0) < 0.05, (taps, f.std(), want)
    assert abs(np.corrcoef(sx.reshape(-1), sy.reshape(-1))[0, 1]) < 0.05                    # the two axes are independent words


def _desc(kind, c=3, **params):
    return aug.photometric_descs(aug.Stage(kind, dict(params, entry=0), None), 10, 10, c)


def test_descriptors_of_the_new_stages():
    assert _desc("median_blur", k=3) == {"mode": pe.MEDIAN, "flags": 0, "seed": 0, "p": [3]}
    assert _desc("median_blur", k=11, c=1) == {"mode": pe.MEDIAN, "flags": 0, "seed": 0, "p": [11]}
    assert _desc("hue_saturation", value=-20) == {"mode": pe.HSV, "flags": 0, "seed": 0, "p": [-20, -20]}
    assert _desc("hue_saturation", value=20)["p"] == [20, 20]
    assert _desc("hue_saturation", value=20, c=1) is None
    assert _desc("elastic", applied=False, sigma=0.25) is None
    assert _desc("elastic", applied=True, alpha=0.5, sigma=0.25, seed=9) == {"mode": pe.ELASTIC, "flags": 0, "seed": 9, "p": [128, 16374, 5]}
    assert _desc("elastic", applied=True, alpha=3.5, sigma=0.25, seed=2 ** 64 - 1, c=1) == {"mode": pe.ELASTIC, "flags": 0, "seed": 2 ** 64 - 1,
                                                                                          "p": [896, 16374, 5]}
    assert aug.elastic_taps(0.25) == (16374, 5)
    w0, w1 = aug.elastic_taps(0.37)
    assert w0 + 2 * w1 == 16384 and w1 > 5
    for sigma in (0.38, 1.0, 0.12, 0.0):                                  # int(4 sigma + 0.5) is 2, 4, 0, 0: not the 3-tap filter
        with pytest.raises(ValueError):
            aug.elastic_taps(sigma)
    with pytest.raises(ValueError):
        _desc("elastic", applied=True, alpha=1.0, sigma=1.0, seed=1)
    assert aug.PHOTO_DESC.itemsize == 136 and _lib.ABI_VERSION == 3
    assert set(aug.PHOTO_POINTWISE) == {po.AFFINE, po.GREY, po.NOISE, po.DROPOUT, pe.HSV}
