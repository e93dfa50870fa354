"""CPU: the oracle of the multi-scale tests (tests/multiscale_oracle.py).  At the sizes the multi-scale model accepts -- sides that
are multiples of 4 * 2**P -- TF1's legacy bilinear resize, restated in its general form, IS the plain slice x[:, ::2**s, ::2**s]:
in_size / out_size is exactly 2**s, every sample position is an integer and the interpolation weight is 0.  That is what lets the
device build its pyramid by decimation (and keep uint8 pixels uint8).  At any other size the two differ, so the equality is not
vacuous.  The fp32 mean the device is held to bit for bit is checked against fp64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import multiscale_oracle as mo  # noqa: E402


@pytest.mark.parametrize("power", [1, 2, 3, 4])
def test_general_bilinear_resize_is_decimation_at_accepted_sizes(power):
    rng = np.random.default_rng(power)
    m = 4 << power
    for hh, ww in [(m, m), (m, 2 * m), (3 * m, m), (2 * m, 5 * m)]:       # from the smallest accepted size up
        for c in (1, 3):
            x8 = rng.integers(0, 256, (2, hh, ww, c), dtype=np.uint8)
            xf = (rng.standard_normal((2, hh, ww, c)) * 3).astype(np.float32)
            for x in (x8, xf):
                levels = mo.pyramid_tf1(x, power)
                assert len(levels) == power + 1
                for s, lv in enumerate(levels):
                    want = mo.decimate(x, s).astype(np.float32)
                    assert lv.dtype == np.float32 and lv.shape == want.shape == (2, hh >> s, ww >> s, c)
                    assert np.array_equal(lv.view(np.uint32), want.view(np.uint32)), (power, hh, ww, c, s)


def test_decimation_commutes_with_the_preprocessing():
    """(x - 127.5) / 127.5 is per pixel: the slice of the preprocessed batch is the preprocessed slice, bit for bit"""
    x8 = np.random.default_rng(0).integers(0, 256, (1, 32, 64, 3), dtype=np.uint8)
    pre = lambda a: ((a.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)    # noqa: E731
    for s in (1, 2, 3):
        assert np.array_equal(mo.resize_bilinear_tf1(pre(x8), 32 >> s, 64 >> s), pre(mo.decimate(x8, s)))


@pytest.mark.parametrize("hh,ww,power", [(44, 32, 3), (32, 52, 3), (20, 36, 3), (12, 20, 3)])
def test_general_bilinear_resize_differs_from_decimation_elsewhere(hh, ww, power):
    """a side that is a multiple of 4 (what the single-scale net accepts) but not of 2**P: the size ratio is not 2**P, so sample
    positions fall between pixels or on other pixels than the slice's (or the level sizes do not even match).  (A side that is a
    multiple of 2**P but not of 4 * 2**P still resizes exactly; there the MAPS of the levels no longer nest, which is the other
    half of the size rule.)  The device refuses all such sizes instead of decimating them."""
    assert hh % 4 == 0 and ww % 4 == 0 and (hh % (1 << power) or ww % (1 << power))
    x = (np.random.default_rng(3).standard_normal((1, hh, ww, 1)) * 3).astype(np.float32)
    s = power
    got = mo.resize_bilinear_tf1(x, hh >> s, ww >> s)
    dec = mo.decimate(x, s)[:, :hh >> s, :ww >> s]
    assert got.shape != dec.shape or not np.array_equal(got, dec)
    if got.shape == dec.shape:
        assert np.abs(got - dec).max() > 1e-3


def test_bilinear_restatement_on_hand_values():
    """1-D, 5 -> 2 samples: scale 2.5, positions 0 and 2.5 -> x[0] and the midpoint of x[2], x[3]; 4 -> 3: scale 4/3"""
    x = np.array([1, 2, 4, 8, 16], np.float32).reshape(1, 1, 5, 1)
    assert mo.resize_bilinear_tf1(x, 1, 2).reshape(-1).tolist() == [1.0, 6.0]
    x = np.array([0, 3, 6, 9], np.float32).reshape(1, 4, 1, 1)
    got = mo.resize_bilinear_tf1(x, 3, 1).reshape(-1)
    assert np.allclose(got, [0.0, 4.0, 8.0], rtol=0, atol=1e-6)         # positions 0, 4/3, 8/3 on a linear ramp of slope 3
    # the last position's hi tap is clamped to the last sample
    x = np.array([5, 7], np.float32).reshape(1, 1, 2, 1)
    assert mo.resize_bilinear_tf1(x, 1, 3).reshape(-1).tolist() == [5.0, np.float32(5) + np.float32(2) * (np.float32(2) / np.float32(3)), 7.0]


def test_upsample_and_fuse_against_fp64():
    rng = np.random.default_rng(11)
    for power in (1, 2, 3, 4):
        for k in (1, 3):
            mh, mw = 2 << power, 3 << power
            levels = [(rng.standard_normal((2, mh >> s, mw >> s, k)) * 10).astype(np.float32) for s in range(power + 1)]
            up = mo.upsample_nearest(levels[power], 2 ** power)
            i, j = rng.integers(0, mh), rng.integers(0, mw)
            assert up.shape == levels[0].shape and np.array_equal(up[:, i, j], levels[power][:, i >> power, j >> power])
            got = mo.fuse_mean_f32(levels)
            ref = mo.fuse_mean_f64(levels)
            assert got.dtype == np.float32 and got.shape == ref.shape == (2, mh, mw, k)
            # P roundings of sums bounded by the sum of |terms| and one of the division: (P + 1) half-ulps of that sum, relative
            bound = (power + 1) * 2.0 ** -24 * sum(np.abs(mo.upsample_nearest(l, 2 ** s)).astype(np.float64)
                                                   for s, l in enumerate(levels)) / (power + 1)
            assert (np.abs(got.astype(np.float64) - ref) <= bound + 1e-300).all()
    # one level: the mean is the level itself
    y = rng.standard_normal((1, 4, 4, 2)).astype(np.float32)
    assert np.array_equal(mo.fuse_mean_f32([y]), y)
    # the order is the stated one: (a + b) + c with a + b rounded first, then the division
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    lv = [np.full((1, 4, 4, 1), a), np.full((1, 2, 2, 1), b), np.full((1, 1, 1, 1), c)]
    assert np.all(mo.fuse_mean_f32(lv) == np.float32(np.float32(np.float32(a + b) + c) / np.float32(3)))
    assert np.float32(np.float32(a + b) + c) != np.float32(a + np.float32(b + c))


def test_sizes_and_refusals_of_the_layer_entry_points_need_no_device():
    """ubd_multiscale_levels_bytes is host arithmetic, and ubd_multiscale_gather / ubd_multiscale_fuse check every argument before
    their first HIP call: a refusal returns non-zero with its message and launches nothing, with or without a GPU"""
    import ctypes
    from ubdvss_amd import _lib
    lib = _lib.load()
    size = lib.ubd_multiscale_levels_bytes
    for n, hh, ww, px, power in [(2, 32, 32, 3, 3), (3, 64, 160, 12, 3), (1, 64, 128, 1, 4), (5, 8, 24, 4, 1)]:
        for first in (0, 1):
            assert size(n, hh, ww, px, first, power) == sum(n * (hh >> s) * (ww >> s) * px for s in range(first, power + 1))
        for s in range(1, power + 1):                                   # where level s starts in a buffer packed from level 1
            assert size(n, hh, ww, px, 1, s - 1) == sum(n * (hh >> t) * (ww >> t) * px for t in range(1, s))
    assert size(1, 32, 32, 3, 1, 0) == 0                                # no level between 1 and 0
    assert size(1, 32, 32, 3, 1, 5) == 0 and size(1, 32, 32, 3, 1, -1) == 0 and size(1, 44, 32, 3, 1, 3) == 0
    assert size(0, 32, 32, 3, 1, 1) == 0 and size(1, 32, 32, 0, 1, 1) == 0 and size(1, 32, 32, 3, -1, 1) == 0
    p = ctypes.c_void_p(4096)                                           # never dereferenced: every call below is refused
    gather, fuse, err = lib.ubd_multiscale_gather, lib.ubd_multiscale_fuse, lib.ubd_last_error
    assert gather(p, _lib.UBD_IN_U8, 1, 48, 32, 3, 3, p, 1 << 20, None) != 0 and b"multiples of 32" in err()
    assert gather(p, _lib.UBD_IN_U8, 1, 36, 32, 3, 1, p, 1 << 20, None) != 0 and b"multiples of 8" in err()
    assert gather(p, _lib.UBD_IN_U8, 1, 64, 64, 3, 5, p, 1 << 20, None) != 0 and b"outside 0..4" in err()
    assert gather(p, _lib.UBD_IN_U8, 1, 64, 64, 3, -1, p, 1 << 20, None) != 0 and b"outside 0..4" in err()
    assert gather(p, _lib.UBD_IN_U8, 1, 64, 64, 3, 0, p, 1 << 20, None) != 0 and b"no levels" in err()
    assert gather(p, _lib.UBD_IN_U8, 1, 64, 64, 2, 1, p, 1 << 20, None) != 0 and b"channels" in err()
    assert gather(p, 7, 1, 64, 64, 3, 1, p, 1 << 20, None) != 0 and b"in_dtype" in err()
    assert gather(p, _lib.UBD_IN_U8, 1, 64, 64, 3, 1, p, 3071, None) != 0 and b"too small (3071 < 3072)" in err()
    assert gather(ctypes.c_void_p(4100), _lib.UBD_IN_U8, 1, 64, 64, 3, 1, p, 1 << 20, None) != 0 and b"16-byte aligned" in err()
    assert gather(None, _lib.UBD_IN_U8, 1, 64, 64, 3, 1, p, 1 << 20, None) != 0 and b"null" in err()
    assert fuse(p, 1, 12, 8, 1, 3, p, None) != 0 and b"multiples of 8" in err()
    assert fuse(p, 1, 8, 8, 1, 5, p, None) != 0 and b"outside 0..4" in err()
    assert fuse(p, 1, 8, 8, 33, 1, p, None) != 0 and b"k must be 1..32" in err()
    assert fuse(p, 1, 8, 8, 1, 1, None, None) != 0 and b"null" in err()
    assert fuse(ctypes.c_void_p(4098), 1, 8, 8, 1, 1, p, None) != 0 and b"misaligned" in err()
    assert lib.ubd_forward_multiscale_workspace_bytes(None, _lib.UBD_IN_U8, 1, 64, 64, 3) == 0
    assert lib.ubd_forward_multiscale(None, p, p, _lib.UBD_IN_U8, 0, 1, 64, 64, 3, p, p, 1 << 20, None) != 0 and b"null" in err()
