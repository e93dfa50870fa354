"""CPU: the numpy restatement of ubd_extract_objects (tests/object_patches_oracle.py) against the installed Pillow, bit for bit;
its orientation rule and its rescale on known answers; and the registration of the entry point (signature table, exported
symbol, ModelRunner.predict_patches refusing to run without a GPU)."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import object_patches_oracle as opo  # noqa: E402


def _random_case(rng):
    h, w = int(rng.integers(1, 61)), int(rng.integers(1, 61))
    c = int(rng.choice([1, 3]))
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    ph, pw = int(rng.integers(1, 41)), int(rng.integers(1, 21))
    if rng.integers(0, 2):
        ph, pw = pw, ph                                  # 1..40 x 1..20, either way round
    if rng.integers(0, 2):
        pts = [(float(rng.integers(-8, w + 9)), float(rng.integers(-8, h + 9))) for _ in range(4)]
    else:
        pts = [(float(rng.uniform(-8, w + 8)), float(rng.uniform(-8, h + 8))) for _ in range(4)]
    return img, pts, ph, pw


def test_oracle_sampler_equals_pillow_quad_bilinear():
    """quad_data + sample == Image.transform((pw, ph), QUAD, nw + sw + se + ne, BILINEAR), every byte, no tolerance"""
    rng = np.random.default_rng(2024)
    n_bytes = 0
    for case in range(80):
        img, (nw, ne, se, sw), ph, pw = _random_case(rng)
        pil = Image.fromarray(img[:, :, 0], "L") if img.shape[2] == 1 else Image.fromarray(img, "RGB")
        want = np.asarray(pil.transform((pw, ph), Image.QUAD, nw + sw + se + ne, Image.BILINEAR)).reshape(ph, pw, -1)
        got = opo.sample(img, opo.quad_data([nw, ne, se, sw], pw, ph), pw, ph)
        assert np.array_equal(got, want), (case, img.shape, (nw, ne, se, sw), (ph, pw), int((got != want).sum()))
        n_bytes += want.size
    assert n_bytes > 20000


def _image(seed, h, w, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def test_wide_box_is_the_crop_from_every_start_and_direction():
    img = _image(1, 30, 40)
    x0, y0, x1, y1 = 5, 7, 29, 16                         # 24 wide, 9 high
    tl, tr, br, bl = (x0, y0), (x1, y0), (x1, y1), (x0, y1)
    crop = img[y0:y1, x0:x1]
    for name, order in (("clockwise from bottom-left", [bl, tl, tr, br]), ("clockwise from top-left", [tl, tr, br, bl]),
                        ("counter-clockwise from top-left", [tl, bl, br, tr])):
        quad = [v for p in order for v in p]
        patch, pq = opo.extract(img, quad, y1 - y0, x1 - x0)
        assert np.array_equal(patch, crop), name
        assert pq in ([*tl, *tr, *br, *bl], [*br, *bl, *tl, *tr]), (name, pq)
    # from the bottom-left the long side comes second (r = 1) and from the top-left first (r = 0): both upright, not the half turn
    assert opo.orient([bl, tl, tr, br]) == [tl, tr, br, bl]
    assert opo.orient([tl, tr, br, bl]) == [tl, tr, br, bl]
    assert opo.orient([tl, bl, br, tr]) == [tl, tr, br, bl]


def test_tall_box_is_a_rotation_never_a_mirror():
    img = _image(2, 40, 30)
    x0, y0, x1, y1 = 4, 3, 13, 33                         # 9 wide, 30 high
    tl, tr, br, bl = (x0, y0), (x1, y0), (x1, y1), (x0, y1)
    crop = img[y0:y1, x0:x1]
    for order in ([tl, tr, br, bl], [tl, bl, br, tr], [br, bl, tl, tr]):
        patch, _ = opo.extract(img, [v for p in order for v in p], x1 - x0, y1 - y0)
        assert patch.shape == (9, 30, 3)
        assert np.array_equal(patch, np.rot90(crop, 3)) or np.array_equal(patch, np.rot90(crop, 1))
        assert not np.array_equal(patch, crop.transpose(1, 0, 2))                 # the mirror image
    patch, _ = opo.extract(img, [*bl, *tl, *tr, *br], x1 - x0, y1 - y0)       # clockwise from the bottom-left: the long side comes first
    assert np.array_equal(patch, np.rot90(crop, 3))
    patch, _ = opo.extract(img, [*tl, *tr, *br, *bl], x1 - x0, y1 - y0)       # from the top-left: the other long side, the half turn
    assert np.array_equal(patch, np.rot90(crop, 1))


def test_tie_square_takes_the_first_side():
    sq = [(2, 3), (12, 3), (12, 13), (2, 13)]
    assert opo.orient(sq) == sq                           # e01 == e12: r = 0
    assert opo.orient(sq[1:] + sq[:1]) == sq[1:] + sq[:1]
    tilted = [(10, 0), (20, 10), (10, 20), (0, 10)]       # a tie again, rotated by 45 degrees
    assert opo.orient(tilted) == tilted
    assert opo.orient([tilted[0], tilted[3], tilted[2], tilted[1]]) == tilted    # counter-clockwise: reversed first


def test_reversing_the_vertex_order_leaves_the_patch_unchanged():
    rng = np.random.default_rng(9)
    img = _image(3, 48, 64)
    for case in range(40):
        q = rng.integers(-8, 72, 8)
        if case % 4 == 0:
            q[6:8] = q[0:2]                               # degenerate ones too
        if case % 8 == 0:
            q[2:4] = q[0:2]; q[4:6] = q[0:2]
        rev = np.concatenate([q[0:2], q[6:8], q[4:6], q[2:4]])
        a, qa = opo.extract(img, q, 7, 19, expand=1.25)
        b, qb = opo.extract(img, rev, 7, 19, expand=1.25)
        area2 = sum(int(q[2 * k]) * int(q[(2 * k + 3) % 8]) - int(q[(2 * k + 2) % 8]) * int(q[2 * k + 1]) for k in range(4))
        if area2 != 0:                                    # a zero area is "clockwise" in both orders: no reversal to undo
            assert qa == qb, case
            assert np.array_equal(a, b), case


def test_rescale_truncates_toward_zero_and_clamps():
    from ubdvss_amd import utils
    q = [-3, 5, 7, -9, -1, -1, 10, 11]
    got = opo.rescale(q, 2.5, 0.75)
    assert got == [(-7, 3), (17, -6), (-2, 0), (25, 8)]   # -7.5 -> -7, -6.75 -> -6, -0.75 -> 0: toward zero, not floor
    assert [v for p in got for v in p] == list(utils.rescale_bbox(q, 2.5, 0.75))
    big = opo.rescale([2 ** 31 - 1, -2 ** 31, 5, 5, 0, 0, 1, 1], 4.0, 4.0)
    assert big[0] == (2 ** 30, -2 ** 30) and big[1] == (20, 20)
    assert opo.rescale(q) == [(-3, 5), (7, -9), (-1, -1), (10, 11)]


def test_expand_is_about_the_mean_and_exact_at_one():
    c = [(0, 0), (8, 0), (8, 4), (0, 4)]
    assert opo.expand_corners(c, 1.0) == [(0.0, 0.0), (8.0, 0.0), (8.0, 4.0), (0.0, 4.0)]
    assert opo.expand_corners(c, 1.5) == [(-2.0, -1.0), (10.0, -1.0), (10.0, 5.0), (-2.0, 5.0)]


def test_entry_point_is_registered_and_exported():
    from ubdvss_amd import _lib
    assert "ubd_extract_objects" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ubd_extract_objects"][1]) == 16
    assert hasattr(_lib.load(), "ubd_extract_objects")


def test_predict_patches_needs_a_gpu():
    import torch
    import ubdvss_amd
    from ubdvss_amd import ModelRunner, NetConfig
    assert callable(ubdvss_amd.extract_objects_on_device)
    runner = ModelRunner(NetConfig(grey=False))
    if torch.cuda.is_available():
        return                                            # the GPU tests run it
    with pytest.raises(RuntimeError):
        runner.predict_patches(None, [np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(RuntimeError):
        ubdvss_amd.extract_objects_on_device([np.zeros((8, 8, 3), np.uint8)], np.zeros((1, 1, 8), np.int32), np.zeros(1, np.int32))
