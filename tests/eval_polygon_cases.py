"""Seeded inputs of the polygon evaluation tests (helper module, not collected): 6 images whose ground truth is the hulls
(9..64 vertices) of rotated rectangles, small ellipses and one chamfered box on a 128 x 160 segmentation map, and whose found
objects are the integer quads the postprocess finds on a perturbed quarter-scale copy of that map (scale 4).  Everything here
runs on the CPU through oracle/cv_post.c; the GPU test requires ubd_segmap_polygons to reproduce the hulls first.

Kinds of image: separate shapes found one by one (one-to-one); a long bar whose quarter-scale copy is cut in two or three
(one-to-many); two shapes a few pixels apart that the quarter-scale copy joins (many-to-one); and a chamfered axis-aligned box on
multiples of 4, whose found box is its bounding box: four found edges collinear with hull edges.
"""
import numpy as np

import segmap_cases as sc
from oracle import cv_post

H, W, SCALE = 128, 160, 4
# the committed seed: with it every exact IoU keeps 1e-6 clear of 0.05 and of the twelve thresholds, with and without SCALES, and no
# group union has more than 6 polygons (tests/test_evaluation_polygons_host.py asserts both with the exact oracle)
SEED = 7
SCALES = [(1.0, 1.0), (1.03125, 0.96875), (0.96875, 1.0), (1.0, 1.03125), (1.015625, 1.015625), (0.984375, 0.96875)]


def _pool(mask, need=1):
    """quarter-scale copy: a map pixel is set when at least ``need`` of its 4 x 4 image pixels are"""
    return (mask.reshape(H // SCALE, SCALE, W // SCALE, SCALE).sum(axis=(1, 3)) >= need)


def _shape(rng, cx, cy, big):
    if rng.integers(2):
        return sc.rotated_rect_mask(H, W, cx, cy, rng.uniform(14, 26) if big else rng.uniform(9, 16), rng.uniform(6, 11), rng.uniform(0.15, np.pi - 0.15))
    return sc.ellipse_mask(H, W, cx, cy, rng.uniform(12, 22), rng.uniform(8, 13), rng.uniform(0, np.pi))


def _image(rng, kind):
    """(segmentation map uint8 (H, W), quarter-scale map uint8)"""
    m = np.zeros((H, W), bool)
    if kind == 0:                                   # separate shapes, found one by one
        for cx, cy in ((35, 32), (115, 40), (60, 96), (130, 100)):
            m |= _shape(rng, cx + rng.uniform(-6, 6), cy + rng.uniform(-6, 6), True)
        q = _pool(m, int(rng.integers(1, 9)))
    elif kind == 1:                                 # a long bar cut into pieces on the quarter-scale map, and a shape nobody found
        ang = rng.uniform(0.08, 0.2) * (1 if rng.integers(2) else -1)     # never axis-aligned: its hull keeps at least 9 vertices
        m |= sc.rotated_rect_mask(H, W, 80, 40, 62, 9, ang)
        m |= _shape(rng, 40, 100, False)
        other = _shape(rng, 120, 100, False)
        q = _pool(m)
        m |= other                                  # missed
        for c in sorted(int(v) for v in rng.choice(np.arange(10, 30), int(rng.integers(1, 3)), replace=False)):
            q[:16, c] = False
    elif kind == 2:                                 # two shapes the quarter-scale map joins, a false positive beside them
        ang = rng.uniform(0.05, 0.1) * (1 if rng.integers(2) else -1)
        m |= sc.rotated_rect_mask(H, W, 45, 50, 28, 11, ang)
        m |= sc.rotated_rect_mask(H, W, 110, 50, 30, 11, ang)
        q = _pool(m)
        q[10:15, 15:24] = True                      # the bridge
        q[26:30, 5:14] = True                       # found where nothing is
        m |= _shape(rng, 110, 100, False)
        q |= _pool(_shape(rng, 110, 100, False))
    else:                                           # chamfered box on multiples of 4: the found box is its bounding box
        x0, y0, x1, y1 = 24, 20, 120, 64
        for k, inset in enumerate((9, 5, 2, 1, 0)):  # rounded corners: a hull of 20 vertices whose four long edges lie on the bounding box
            m[y0 + k:y1 + 1 - k, x0 + inset:x1 + 1 - inset] = True
        m |= sc.ellipse_mask(H, W, 80 + rng.uniform(-3, 3), 98, 54, 24, rng.uniform(-0.05, 0.05))   # a large ellipse: the most vertices
        q = _pool(m)
    return m.astype(np.uint8) * 255, q.astype(np.uint8)


def images(seed=SEED):
    """list of (segmentation map, quarter-scale map): kinds 0, 1, 2, 3, 0, 1"""
    rng = np.random.default_rng(seed)
    return [_image(rng, kind) for kind in (0, 1, 2, 3, 0, 1)]


def ground_truth(seg_map):
    """hulls of at least 3 vertices as flat int lists, in the reader's order"""
    return [[int(v) for v in p.reshape(-1)] for p in sc.expected_polygons(seg_map) if len(p) >= 3]


def found_quads(quarter_map):
    quads, _ = cv_post.postprocess(quarter_map, None, scale=SCALE, min_area_threshold=1)
    return [[int(v) for v in q] for q in quads]


def batch(seed=SEED):
    """list of (gts, founds) images, the layout of tests/eval_cases.batch"""
    return [(ground_truth(m), found_quads(q)) for m, q in images(seed)]


def scaled(imgs, scales=SCALES):
    """the batch as the device sees it with ``scales``: found coordinate = int(coordinate * scale) (utils.py:67-69)"""
    return [(g, [[int(v * (s[0] if k % 2 == 0 else s[1])) for k, v in enumerate(q)] for q in f]) for (g, f), s in zip(imgs, scales)]
