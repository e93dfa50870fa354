"""CPU: the host half of the mask-blended augmentation stages (SimplexNoiseAlpha, FrequencyNoiseAlpha) of
ubdvss_amd/augmentation.py: the noise grids, the curve, the coarse-size rule, the draws behind ``noise_alpha=True`` and the
lowering to the descriptor of ubd_noise_alpha_images."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import noise_alpha_oracle as no  # noqa: E402
from ubdvss_amd import _lib  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

SHAPES = [(1, 1), (1, 16), (16, 1), (2, 3), (7, 5), (16, 16)]


@pytest.mark.parametrize("make", [aug.simplex_grid, lambda gh, gw, seed: aug.frequency_grid(gh, gw, -2.5, seed)])
def test_grids(make):
    for gh, gw in SHAPES:
        g = make(gh, gw, 11)
        assert g.shape == (gh, gw) and g.dtype == np.uint16 and int(g.max()) <= 32768
        assert np.array_equal(g, make(gh, gw, 11))
        if gh * gw > 1:
            assert len(np.unique(g)) > 1, (gh, gw)
            assert not np.array_equal(g, make(gh, gw, 12)), (gh, gw)
    assert aug.frequency_grid(1, 1, -2.5, 3)[0, 0] == 16384                # a constant field becomes 0.5
    assert aug.simplex_grid(1, 1, 3)[0, 0] == 16384                        # simplex noise is 0 at the origin


def test_frequency_grid_equals_a_direct_inverse_dft():
    gh = gw = 4
    for seed, exponent in ((5, -3.0), (6, -0.5), (7, 0.0)):
        r, a = np.random.default_rng(seed).random((2, gh, gw))
        fy, fx = np.fft.fftfreq(gh), np.fft.fftfreq(gw)
        g = np.zeros((gh, gw), np.float64)
        for y in range(gh):
            for x in range(gw):
                acc = 0j
                for v in range(gh):
                    for u in range(gw):
                        if (u, v) != (0, 0):
                            f = np.sqrt(fx[u] ** 2 + fy[v] ** 2)
                            acc += r[v, u] * f ** exponent * np.exp(2j * np.pi * a[v, u]) * np.exp(2j * np.pi * (u * x / gw + v * y / gh))
                g[y, x] = (acc / (gh * gw)).real
        g = (g - g.min()) / (g.max() - g.min())
        got = aug.frequency_grid(gh, gw, exponent, seed).astype(np.int64)
        assert np.abs(got - np.rint(32768.0 * g)).max() <= 1, (seed, exponent)


def test_alpha_curve():
    for thr in (-12.0, -3.0, 0.0, 4.5, 15.0):
        t = aug.alpha_curve(True, thr)
        assert t.shape == (257,) and t.dtype == np.uint16 and int(t.max()) <= 16384
        assert (np.diff(t.astype(np.int64)) >= 0).all()
    assert aug.alpha_curve(True, 0.0)[128] == 8192
    assert np.array_equal(aug.alpha_curve(False, 3.0), 64 * np.arange(257))


def test_coarse_size_rule():
    f = aug.noise_alpha_grid_size                                         # (h, w, size_px_max) -> (gh, gw)
    assert f(512, 512, 8) == (8, 8)                                       # square
    assert f(100, 400, 16) == (4, 16) and f(64, 4000, 8) == (1, 8)        # wide: the short side keeps the aspect, at least 1
    assert f(400, 100, 16) == (16, 4) and f(300, 200, 9) == (9, 6)        # tall
    assert f(3, 5, 8) == (3, 5) and f(1, 1, 2) == (1, 1)                  # tiny: no larger than the limit, the image's own size
    assert f(20, 30, 40) == (16, 16) and f(4, 40, 64) == (4, 16)          # the clamp to 16 cells
    assert aug.NOISE_ALPHA_MAX_GRID == 16


def _draw(seed, **kw):
    return aug.sample_photometric(3, np.random.default_rng(seed), **kw)


# sha256 over repr(sample_photometric(3, default_rng(seed), extended)) for seed 0..499, taken from the sampler as it was before the
# noise_alpha flag existed (repr of a float is its shortest round-trip form: the digest pins every drawn number)
DIGEST_BEFORE = {False: "0e2547746d4ba6dd1867f35caf6d2eacf5f3abe4c908f800243d9065eb3fac54",
                 True: "9dbec1d5ddc4b9a337381c90a574a61c1a8b4baa365fc8f77c6bbf196fe2fc43"}


def test_without_the_flag_every_draw_is_as_before():
    assert aug.PHOTO_NOISE_ALPHA == ("SimplexNoiseAlpha", "FrequencyNoiseAlpha")
    for extended in (False, True):
        h = hashlib.sha256()
        for seed in range(500):
            h.update(repr(aug.sample_photometric(3, np.random.default_rng(seed), extended)).encode())
        assert h.hexdigest() == DIGEST_BEFORE[extended]
    for seed in range(500):
        for extended in (False, True):
            plain = _draw(seed, extended=extended)
            assert plain == _draw(seed, extended=extended, noise_alpha=False)
            assert not any(st.kind in aug.NOISE_ALPHA_KINDS for st in plain)
            # the two operations still come out as unbuilt, as often as the flag would draw them
            flagged = _draw(seed, extended=extended, noise_alpha=True)
            assert len(flagged) == len(plain) and [st.params["entry"] for st in flagged] == [st.params["entry"] for st in plain]
            for p, q in zip(plain, flagged):
                if q.kind in aug.NOISE_ALPHA_KINDS:
                    assert p.kind == "unbuilt" and p.params["name"] == aug.PHOTO_NOISE_ALPHA[aug.NOISE_ALPHA_KINDS.index(q.kind)]
                    break                                                 # later stages draw from a moved stream
                assert p == q


def test_with_both_flags_nothing_is_unbuilt_and_every_choice_occurs():
    kinds, methods, aggs, sigmoids, directed, sizes = set(), set(), set(), set(), set(), {k: set() for k in aug.NOISE_ALPHA_KINDS}
    gen = np.random.default_rng(77)
    for _ in range(2000):
        for st in aug.sample_photometric(3, gen, extended=True, noise_alpha=True):
            assert st.kind != "unbuilt"
            if st.kind in aug.NOISE_ALPHA_KINDS:
                q = st.params
                kinds.add(st.kind)
                assert 1 <= len(q["iterations"]) <= 3
                for it in q["iterations"]:
                    methods.add(it["upscale"])
                    sizes[st.kind].add(it["size"])
                    assert 0 <= it["seed"] < 2 ** 64
                if st.kind == "simplex_alpha":
                    assert q["aggregation"] == "max" and q["sigmoid"] is True and 0.5 <= q["alpha"] <= 1.0
                    directed.add(q["directed"])
                    assert ("direction" in q) == q["directed"]
                else:
                    aggs.add(q["aggregation"])
                    sigmoids.add(q["sigmoid"])
                    assert -4.0 <= q["exponent"] <= 0.0 and len(q["factors"]) == 3 and all(0.5 <= f <= 1.5 for f in q["factors"])
                    assert 0.5 <= q["contrast_alpha"] <= 2.0
    assert kinds == set(aug.NOISE_ALPHA_KINDS) and methods == {"nearest", "linear", "cubic"}
    assert aggs == {"avg", "max"} and sigmoids == {False, True} and directed == {False, True}
    assert sizes["simplex_alpha"] == set(range(2, 17)) and sizes["frequency_alpha"] == set(range(4, 17))


def test_the_stages_before_the_first_new_one_equal_the_plain_draw():
    seen = 0
    for seed in range(400):
        plain, both = _draw(seed, extended=True), _draw(seed, extended=True, noise_alpha=True)
        assert len(plain) == len(both)
        for p, q in zip(plain, both):
            if q.kind in aug.NOISE_ALPHA_KINDS:
                seen += 1
                break
            assert p == q
        else:
            assert plain == both
    assert seen > 50
    # the flags are independent: noise_alpha alone leaves the three extended operations unbuilt
    names = {st.params["name"] for seed in range(300) for st in _draw(seed, noise_alpha=True) if st.kind == "unbuilt"}
    assert names == set(aug.PHOTO_EXTENDED)


def test_sample_plan_threads_the_flag():
    import random
    from ubdvss_amd import ObjectMarkup
    mk = [ObjectMarkup([30, 25, 60, 25, 60, 45, 30, 45])]
    hit = False
    for seed in range(200):
        args = lambda: ((90, 70), mk, random.Random(seed), np.random.RandomState(seed), np.random.default_rng(seed))  # noqa: E731
        a, b = aug.sample_plan(*args(), photo_extended=True), aug.sample_plan(*args(), photo_extended=True, photo_noise_alpha=False)
        assert a == b
        c = aug.sample_plan(*args(), True, True)                          # positional: appended after photo_extended
        assert c.stages == a.stages and not any(st.kind == "unbuilt" for st in c.photometric)
        hit = hit or any(st.kind in aug.NOISE_ALPHA_KINDS for st in c.photometric)
    assert hit


def test_directed_edge_kernel_and_the_tap_limits():
    rng = np.random.default_rng(4)
    for d in list(rng.uniform(0, 1, 50)) + [0.0, 0.25, 0.5, 0.75, 1.0]:
        m = aug.directed_edge_kernel(d)
        assert abs(m.sum()) < 1e-12 and m[1, 1] == 1.0 and (np.delete(m.reshape(-1), 4) <= 0).all()
    # direction 0: the vector points up (y = -1 in image coordinates): the cell above weighs most
    m = aug.directed_edge_kernel(0.0)
    assert np.argmin(np.delete(m.reshape(-1), 4)) == 1
    St = aug.Stage
    its = ({"size": 8, "upscale": "cubic", "seed": 1},)
    for alpha in (0.5, 0.77, 1.0):
        for directed, d in ((False, None), (True, 0.0), (True, 0.13), (True, 0.5), (True, 0.999)):
            q = {"directed": directed, "alpha": alpha, "iterations": its, "aggregation": "max", "sigmoid": True, "threshold": 0.0}
            if directed:
                q["direction"] = d
            f, tab = aug.noise_alpha_descs(St("simplex_alpha", q, None), 40, 30, 3)
            taps = np.array(f["first"]["p"])
            assert f["first"]["kind"] == _lib.UBD_NA_FILTER3 and f["second"]["kind"] == _lib.UBD_NA_IDENTITY
            assert taps.shape == (9,) and np.abs(taps).max() <= 13 * 16384
            assert abs(int(taps.sum()) - int(np.rint((1.0 - alpha) * 16384))) <= 5      # E sums to 0: the taps sum to 1 - alpha
            if not directed:
                assert list(taps) == [int(np.rint(v * 16384)) for v in (0, alpha, 0, alpha, 1 - 5 * alpha, alpha, 0, alpha, 0)]


def test_lowering_of_both_kinds():
    St = aug.Stage
    its = ({"size": 4, "upscale": "nearest", "seed": 9}, {"size": 16, "upscale": "linear", "seed": 10}, {"size": 7, "upscale": "cubic", "seed": 11})
    q = {"exponent": -2.0, "factors": (0.5, 1.0, 1.5), "contrast_alpha": 2.0, "iterations": its, "aggregation": "avg", "sigmoid": False,
         "threshold": 1.0}
    for c in (1, 3):
        f, tab = aug.noise_alpha_descs(St("frequency_alpha", q, None), 200, 100, c)
        assert tab.dtype == np.uint16 and tab.size == 2 * 4 + 8 * 16 + 3 * 7 + 257
        assert [(g["gh"], g["gw"], g["upscale"], g["grid_offset"]) for g in f["grids"]] == [(2, 4, 0, 0), (8, 16, 1, 8), (3, 7, 2, 136)]
        assert f["curve_offset"] == 157 and f["aggregation"] == _lib.UBD_NA_AVG
        assert np.array_equal(tab[157:], 64 * np.arange(257)) and int(tab[:157].max()) <= 32768
        assert np.array_equal(tab[8:136].reshape(8, 16), aug.frequency_grid(8, 16, -2.0, 10))
        # the formulas of photometric_descs for multiply and contrast
        mul = aug.photometric_descs(St("multiply", {"factors": (0.5, 1.0, 1.5), "per_channel": True}, None), 8, 8, c)
        con = aug.photometric_descs(St("contrast", {"alphas": (2.0, 2.0, 2.0), "per_channel": False}, None), 8, 8, c)
        assert f["first"] == {"kind": _lib.UBD_NA_AFFINE, "p": mul["p"]} and f["second"] == {"kind": _lib.UBD_NA_AFFINE, "p": con["p"]}
        d = np.zeros(1, aug.NOISE_ALPHA_DESC)
        aug.fill_noise_alpha_desc(d[0], f, 1000)
        assert d[0]["iterations"] == 3 and d[0]["curve_offset"] == 1157 and list(d[0]["grid"]["grid_offset"]) == [1000, 1008, 1136]
        assert list(d[0]["first"]["p"][:6]) == mul["p"] and d[0]["second"]["kind"] == 2
        img = np.random.default_rng(c).integers(0, 256, (100, 200, c), dtype=np.uint8)
        out = no.apply_fields(img, f, tab)                                # the oracle takes what the lowering makes
        assert out.shape == img.shape and not np.array_equal(out, img)
    assert aug.NOISE_ALPHA_DESC.itemsize == 192
    # photometric_descs keeps its contract for the kinds it knows and raises for the two it does not lower
    for kind in aug.NOISE_ALPHA_KINDS:
        with pytest.raises(ValueError, match="noise_alpha_descs"):
            aug.photometric_descs(St(kind, {}, None), 8, 8, 3)
    assert aug.photometric_descs(St("unbuilt", {"name": "SimplexNoiseAlpha"}, None), 8, 8, 3) is None


def test_oracle_known_answers():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    g = rng.integers(0, 32769, (3, 7))
    taps = [0, 8192, 0, 8192, -16384, 8192, 0, 8192, 0]
    ident, ones, zeros = 64 * np.arange(257), np.full(257, 16384), np.zeros(257, np.int64)
    for up in (no.NEAREST, no.LINEAR, no.CUBIC):
        u = no.upscale(g, 9, 13, up)
        assert u.min() >= 0 and u.max() <= 32768
        assert np.array_equal(no.upscale(np.full((3, 7), 12345), 9, 13, up), np.full((9, 13), 12345))      # the weights sum to one
        assert np.array_equal(no.upscale(g, 3, 7, up), g)                # same size: phase 0, the grid itself
        assert np.array_equal(no.apply(img, (no.FILTER3, taps), (no.IDENTITY, []), [(g, up)], no.MAX, ones), no.po.filter3(img, taps))
        assert np.array_equal(no.apply(img, (no.FILTER3, taps), (no.IDENTITY, []), [(g, up)], no.MAX, zeros), img)
        assert np.array_equal(no.apply(img, (no.IDENTITY, []), (no.IDENTITY, []), [(g, up)], no.AVG, ident), img)
    assert np.array_equal(no.keys_weights(np.arange(32)).sum(-1), np.full(32, 131072))
    assert np.abs(no.keys_weights(np.arange(32))).sum(-1).max() == 180224       # 1.375 x 2^17, at k = 16
    # nearest doubles every cell of a 2 x 2 grid on a 4 x 4 image; linear at the pixel centres of a 1 x 2 grid on 1 x 4
    assert np.array_equal(no.upscale([[1, 2], [3, 4]], 4, 4, no.NEAREST), np.kron([[1, 2], [3, 4]], np.ones((2, 2), np.int64)))
    assert list(no.upscale([[0, 32768]], 1, 4, no.LINEAR)[0]) == [0, 8192, 24576, 32768]
