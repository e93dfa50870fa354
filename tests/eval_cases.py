"""Seeded inputs of the evaluation tests (helper module, not collected): per image a list of ground-truth polygons (flat
coordinate lists, 3..8 vertices, either winding) and a list of found quads (integers).  ``quant`` = 1: integer ground truth,
0.25: quarter-pixel ground truth.  Coordinates stay below 2^14."""
import math

import numpy as np

# the committed seeds: with them no pair, group or by-area IoU lies within 1e-9 of 0.05 or of a threshold (asserted by
# tests/test_gpu_evaluation.py with the exact oracle; the number of excluded cases is zero)
SEED_INT = 11
SEED_QUARTER = 23
SEED_CLASSES = 5


def _q(v, quant):
    return float(np.round(v / quant) * quant)


def _convex_ok(p):
    n = len(p) // 2
    pts = [(p[2 * i], p[2 * i + 1]) for i in range(n)]
    sign = 0
    for i in range(n):
        (ax, ay), (bx, by), (cx, cy) = pts[i], pts[(i + 1) % n], pts[(i + 2) % n]
        cr = (bx - ax) * (cy - by) - (by - ay) * (cx - bx)
        if cr == 0:
            return False                       # the generator keeps strictly convex outlines; degenerate ones are listed by hand
        s = 1 if cr > 0 else -1
        if sign and s != sign:
            return False
        sign = s
    return True


def rotated_rect(rng, cx, cy, w, h, angle, quant=1):
    while True:
        c, s = math.cos(angle), math.sin(angle)
        out = []
        for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)):
            out += [_q(cx + dx * c - dy * s, quant), _q(cy + dx * s + dy * c, quant)]
        if _convex_ok(out):
            return out
        angle += 0.01


def convex_gon(rng, k, cx, cy, rx, ry, quant=1):
    while True:
        ang = np.sort(rng.uniform(0, 2 * math.pi, k))
        out = []
        for a in ang:
            out += [_q(cx + rx * math.cos(a), quant), _q(cy + ry * math.sin(a), quant)]
        if _convex_ok(out):
            return out if rng.integers(2) else _reverse(out)


def _reverse(p):
    n = len(p) // 2
    out = []
    for i in range(n - 1, -1, -1):
        out += [p[2 * i], p[2 * i + 1]]
    return out


def _ints(p):
    return [int(round(v)) for v in p]


def listed_images():
    """Images built by hand for the rules: shared edges, shared vertices, identical polygons, zero-area slivers, every
    class of correspondence.  Integer coordinates."""
    R = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]          # noqa: E731
    imgs = []
    # 0: identical polygon (IoU 1), a found quad sharing an edge with it from outside, one sharing only a corner
    imgs.append(([R(10, 10, 110, 70)], [R(10, 10, 110, 70), R(110, 10, 150, 70), R(110, 70, 130, 90)]))
    # 1: 1-1 below every threshold (IoU 77/323), and a ground truth nobody found
    imgs.append(([R(0, 0, 100, 40), R(300, 300, 340, 330)], [R(50, 3, 150, 43)]))
    # 2: accepted 1-many: two found halves sharing an edge inside the ground truth
    imgs.append(([R(20, 20, 221, 81)], [R(20, 20, 120, 81), R(120, 20, 221, 80)]))
    # 3: rejected 1-many: two small found quads in a large ground truth (group IoU 0.2376...)
    imgs.append(([R(0, 0, 201, 101)], [R(3, 3, 53, 53), R(100, 40, 147, 90)]))
    # 4: accepted many-1: one found quad over two ground truths that share an edge
    imgs.append(([R(10, 10, 111, 61), R(111, 10, 210, 61)], [R(10, 10, 210, 62)]))
    # 5: rejected many-1: one large found quad over two small ground truths
    imgs.append(([R(10, 10, 71, 71), R(200, 10, 261, 71)], [R(0, 0, 300, 81)]))
    # 6: a ground truth touched by two found quads of which one also touches another ground truth: neither kind of group
    imgs.append(([R(0, 0, 101, 50), R(120, 0, 201, 50)], [R(0, 0, 61, 50), R(61, 0, 190, 51)]))
    # 7: no found objects
    imgs.append(([R(5, 5, 50, 50), [60, 60, 90, 60, 75, 93]], []))
    # 8: zero-area slivers among the found quads (collinear, and a repeated vertex pair), beside a rotated 1-1 pair
    imgs.append(([[100, 0, 200, 100, 100, 200, 0, 100]], [[101, 3, 199, 100, 100, 197, 2, 100], [0, 0, 10, 0, 20, 0, 10, 0],
                                                           [50, 50, 50, 50, 70, 70, 70, 70]]))
    # 9: rectangle against its 45-degree turn; octagon ground truth clockwise; triangle sharing a vertex with the quad
    imgs.append(([_reverse([30, 0, 70, 0, 100, 30, 100, 70, 70, 100, 30, 100, 0, 70, 0, 30]), [100, 100, 140, 100, 100, 141]],
                 [[50, -20, 120, 50, 50, 120, -20, 50], [3, 3, 97, 3, 97, 98, 3, 98]]))
    return imgs


def random_image(rng, quant):
    gts, founds = [], []
    n_gt = int(rng.integers(1, 5))
    for g in range(n_gt):
        cx, cy = 150 + 330 * g + rng.uniform(-20, 20), rng.uniform(150, 900)
        kind = int(rng.integers(6))
        if rng.integers(2):
            w, h = rng.uniform(60, 260), rng.uniform(30, 120)
            gt = rotated_rect(rng, cx, cy, w, h, rng.uniform(0, math.pi), quant)
        else:
            gt = convex_gon(rng, int(rng.integers(3, 9)), cx, cy, rng.uniform(40, 140), rng.uniform(30, 100), quant)
        gts.append(gt)
        xs, ys = gt[0::2], gt[1::2]
        x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
        if kind <= 1:                          # one found quad around the object, loose or tight
            j = 1 + 12 * kind
            founds.append(_ints([x0 + rng.uniform(-j, j), y0 + rng.uniform(-j, j), x1 + rng.uniform(-j, j), y0 + rng.uniform(-j, j),
                                 x1 + rng.uniform(-j, j), y1 + rng.uniform(-j, j), x0 + rng.uniform(-j, j), y1 + rng.uniform(-j, j)]))
            if not _convex_ok(founds[-1]):
                founds[-1] = _ints([x0, y0, x1, y0, x1, y1, x0, y1])
        elif kind == 2:                        # two or three found pieces that share edges
            cuts = sorted(int(v) for v in rng.uniform(x0 + 10, x1 - 10, int(rng.integers(1, 3))))
            edges = [int(x0)] + cuts + [int(x1) + 1]
            for a, b in zip(edges, edges[1:]):
                if b > a:
                    founds.append([a, int(y0), b, int(y0), b, int(y1) + 1, a, int(y1) + 1])
        elif kind == 3:                        # a rotated found quad across the object
            founds.append(_ints(rotated_rect(rng, cx + rng.uniform(-15, 15), cy + rng.uniform(-15, 15), (x1 - x0) * rng.uniform(0.5, 1.1),
                                             (y1 - y0) * rng.uniform(0.5, 1.1), rng.uniform(0, math.pi), 1)))
        elif kind == 4 and g + 1 < n_gt:       # a found quad reaching towards the next ground truth
            founds.append(_ints([x0, y0, x1 + 250, y0, x1 + 250, y1, x0, y1]))
        # kind 5: missed
    for _ in range(int(rng.integers(0, 3))):   # false positives, sometimes overlapping each other
        founds.append(_ints(rotated_rect(rng, rng.uniform(100, 1400), rng.uniform(1000, 1300), rng.uniform(20, 200), rng.uniform(20, 120),
                                         rng.uniform(0, math.pi), 1)))
    return gts, founds


def batch(seed, quant, n_random=22, with_listed=True):
    """list of (gts, founds) images"""
    rng = np.random.default_rng(seed)
    imgs = listed_images() if with_listed else []
    imgs += [random_image(rng, quant) for _ in range(n_random)]
    return imgs


def tie_image():
    """IoU exactly 1/2 from integer boxes (exactly representable): must be accepted at the threshold 0.5 (>=) and must not
    count for the detection rate there (strict >).  100 x 60 against 100 x 30 inside it."""
    return [[0, 0, 100, 0, 100, 60, 0, 60]], [[0, 0, 100, 0, 100, 30, 0, 30]]
