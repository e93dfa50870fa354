"""CPU oracle of the pixel classification accuracy (helper module of the tests, not collected).

Two independent restatements of the object rule of evaluation.py:546-575 (the reference's
_calc_pixel_classification_correctness_mask: findContours(RETR_EXTERNAL), min_area = -1, drawContours(..., -1)):

* ``objects_contours``: oracle.cv_post.find_contours + fill_contour, the sequential border following and contour fill;
* ``objects_labelling``: scipy.ndimage labelling (foreground 8-connected, background 4-connected), the externality test
  "the pixel north of the component's raster-first pixel is the frame or outside background", and binary_fill_holes.

Both return, per image, the list of (correct, size) of every object as Python ints in raster order of the objects' first
pixels.  Exact sums are ``fractions.Fraction``.  Also here: the seeded case set and the hand-built quirk maps the CPU and
the GPU tests share.
"""
from fractions import Fraction

import numpy as np

SIZES = ((1, 1), (1, 37), (37, 1), (50, 70), (128, 128), (129, 128), (200, 136), (256, 256))
CLASS_COUNTS = (1, 2, 3, 31)


# ---- per-pixel part -----------------------------------------------------------------------------------------------------------------
def classify(class_logits, labels):
    """(h, w, C) logits, (h, w) labels -> (mask bool, correct bool): evaluation.py:553-557 with np.argmax itself"""
    t = np.asarray(labels).astype(np.int64)
    mask = t > 0
    true = np.where(mask, t - 1, 0)
    pred = np.argmax(np.asarray(class_logits), axis=-1)
    return mask, true == pred


def correctness_mask(mask, correct):
    return np.where(mask, np.where(correct, 1, -1), 0).astype(np.int8)


# ---- the object rule, twice -----------------------------------------------------------------------------------------------------------
def objects_contours(mask, correct):
    from oracle import cv_post as ocv
    h, w = mask.shape
    out = []
    for cnt in ocv.find_contours(mask.astype(np.uint8), approx_simple=False):
        region = ocv.fill_contour(cnt, h, w).astype(bool)
        first = int(np.flatnonzero(region.reshape(-1))[0])
        out.append((first, int(np.count_nonzero(correct & region)), int(np.count_nonzero(region))))
    return [(c, s) for _, c, s in sorted(out)]


def objects_labelling(mask, correct):
    from scipy import ndimage
    h, w = mask.shape
    fg, nfg = ndimage.label(mask, structure=np.ones((3, 3), int))
    bg, _ = ndimage.label(~mask)                                                # 4-connected
    frame = np.zeros((h, w), bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    outside = set(np.unique(bg[frame & ~mask]).tolist()) - {0}
    out = []
    for k in range(1, nfg + 1):
        comp = fg == k
        first = int(np.flatnonzero(comp.reshape(-1))[0])
        y, x = divmod(first, w)
        if not (y == 0 or int(bg[y - 1, x]) in outside):                       # north of the first pixel is background by construction
            continue
        region = ndimage.binary_fill_holes(comp)
        out.append((first, int(np.count_nonzero(correct & region)), int(np.count_nonzero(region))))
    return [(c, s) for _, c, s in sorted(out)]


def image_stats(class_logits, labels, objects=objects_contours):
    """one image -> dict(n_correct, n_total, objects [(correct, size)], mask int8 (h, w))"""
    mask, correct = classify(class_logits, labels)
    return dict(n_correct=int(np.count_nonzero(mask & correct)), n_total=int(np.count_nonzero(mask)),
                objects=objects(mask, correct), mask=correctness_mask(mask, correct))


def exact_acc_sum(objects):
    return sum((Fraction(c, s) for c, s in objects), Fraction(0))


def batch_stats(class_logits, labels, objects=objects_contours):
    return [image_stats(class_logits[i], labels[i], objects) for i in range(len(labels))]


# ---- seeded random maps: blobs with holes, nested components, diagonal-only links, isolated pixels, noise patches ---------------
def blob_labels(rng, h, w, n_classes):
    t = np.zeros((h, w), np.int32)
    yy, xx = np.mgrid[0:h, 0:w]

    def ellipse(cy, cx, ry, rx):
        return ((yy - cy) / max(ry, 0.5)) ** 2 + ((xx - cx) / max(rx, 0.5)) ** 2 <= 1.0

    for _ in range(int(rng.integers(1, 3 + h * w // 600))):
        cy, cx = rng.integers(0, h), rng.integers(0, w)
        ry, rx = rng.integers(1, max(2, h // 3 + 1)), rng.integers(1, max(2, w // 3 + 1))
        cls = int(rng.integers(1, n_classes + 1))
        t[ellipse(cy, cx, ry, rx)] = cls
        if rng.random() < 0.7:                                                  # a hole, sometimes with a component nested in it
            t[ellipse(cy, cx, ry * 0.6, rx * 0.6)] = 0
            if rng.random() < 0.6:
                t[ellipse(cy, cx, ry * 0.3, rx * 0.3)] = int(rng.integers(1, n_classes + 1))
                if rng.random() < 0.5:
                    t[ellipse(cy, cx, ry * 0.15, rx * 0.15)] = 0
        if rng.random() < 0.3:                                                  # a second class touching the first
            t[ellipse(cy, min(w - 1, cx + rx), ry * 0.5, rx * 0.5)] = int(rng.integers(1, n_classes + 1))
    for _ in range(int(rng.integers(0, 3 + (h + w) // 40))):                    # diagonal-only chains
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        cls = int(rng.integers(1, n_classes + 1))
        for _ in range(int(rng.integers(2, 12))):
            if 0 <= y < h and 0 <= x < w:
                t[y, x] = cls
            y += 1
            x += 1 if rng.random() < 0.5 else -1
    iso = rng.random((h, w)) < 0.004                                            # isolated pixels
    t[iso] = rng.integers(1, n_classes + 1, size=int(iso.sum()))
    if h * w >= 64 and rng.random() < 0.7:                                      # a noise patch: tiny components, diamonds, pin holes
        ph, pw = min(h, int(rng.integers(2, max(3, h // 3 + 1)))), min(w, int(rng.integers(2, max(3, w // 3 + 1))))
        y0, x0 = int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))
        noise = rng.random((ph, pw)) < 0.5
        t[y0:y0 + ph, x0:x0 + pw] = np.where(noise, rng.integers(1, n_classes + 1, size=(ph, pw)), 0)
    if rng.random() < 0.3:                                                      # frame contact along one side
        t[:, 0] = int(rng.integers(1, n_classes + 1))
    return t


def random_batch(seed, n, h, w, n_classes):
    """labels (n, h, w) int32 and the net-shaped logits (n, h, w, 1 + n_classes) float32: the true class is favoured (about 2 / 3
    of the pixels correct) and the values lie on a grid of 1 / 4, so that exact ties are common"""
    rng = np.random.default_rng(seed)
    labels = np.stack([blob_labels(rng, h, w, n_classes) for _ in range(n)])
    z = rng.normal(size=(n, h, w, 1 + n_classes)).astype(np.float32)
    true = np.where(labels > 0, labels - 1, 0)
    boost = np.zeros_like(z)
    np.put_along_axis(boost, (true + 1)[..., None], 1.5, axis=-1)
    z = np.round((z + boost) * 4) / 4
    return labels.astype(np.int32), z.astype(np.float32)


def seeded_cases():
    """(seed, n, h, w, C) of every case of the committed set: every size with every class count"""
    out = []
    for si, (h, w) in enumerate(SIZES):
        for ci, c in enumerate(CLASS_COUNTS):
            n = 2 if h * w >= 200 * 136 else 3
            out.append((1000 + 10 * si + ci, n, h, w, c))
    return out


# ---- quirk maps: labels (h, w), predicted class per pixel (h, w), expected numbers written out ----------------------------------
def _ring():
    t = np.zeros((5, 5), np.int32)
    t[1:4, 1:4] = 1
    t[2, 2] = 0
    return t


def quirk_maps():
    """name -> (labels, pred, dict(n_correct, n_total, objects)); C = 3 for all of them"""
    q = {}
    # a ring of class 0 around a hole: 8 ring pixels; the hole is "correct" iff it is predicted class 0
    q["ring_hole_pred0"] = (_ring(), np.zeros((5, 5), int), dict(n_correct=8, n_total=8, objects=[(9, 9)]))
    p = np.zeros((5, 5), int)
    p[2, 2] = 1
    q["ring_hole_pred1"] = (_ring(), p, dict(n_correct=8, n_total=8, objects=[(8, 9)]))
    # a component nested in a hole: outer ring 7 x 7 border of the inner 7 x 7 square, a single pixel of class 2 in its middle.
    # ONE object of 49 pixels; pred = 0 everywhere: the 24 ring pixels (class 0) and the 24 hole pixels are correct, the nested pixel is not
    t = np.zeros((9, 9), np.int32)
    t[1:8, 1:8] = 1
    t[2:7, 2:7] = 0
    t[4, 4] = 3
    q["nested_component"] = (t, np.zeros((9, 9), int), dict(n_correct=24, n_total=25, objects=[(48, 49)]))
    # a diamond of four diagonal neighbours encloses its centre (background is 4-connected): one object of 5 pixels
    t = np.zeros((5, 5), np.int32)
    t[1, 2] = t[2, 1] = t[2, 3] = t[3, 2] = 2
    p = np.ones((5, 5), int)                                                     # class 1 everywhere: the four are correct, the centre (true 0) is not
    q["diamond"] = (t, p, dict(n_correct=4, n_total=4, objects=[(4, 5)]))
    # two classes touching are one object
    t = np.zeros((4, 6), np.int32)
    t[1:3, 1:3] = 1
    t[1:3, 3:5] = 2
    q["two_classes_touching"] = (t, np.zeros((4, 6), int), dict(n_correct=4, n_total=8, objects=[(4, 8)]))
    # single pixels are objects; raster order: (0, 0) wrong, (0, 4) right, (2, 2) right
    t = np.zeros((3, 5), np.int32)
    t[0, 0] = 2
    t[0, 4] = 1
    t[2, 2] = 1
    q["single_pixels"] = (t, np.zeros((3, 5), int), dict(n_correct=2, n_total=3, objects=[(0, 1), (1, 1), (1, 1)]))
    # frame contact: a U open to the top edge encloses nothing (its inside is outside background); a ring ON the frame still encloses
    t = np.zeros((4, 5), np.int32)
    t[0:3, 0] = t[0:3, 2] = 1
    t[2, 1] = 1
    q["frame_open_u"] = (t, np.zeros((4, 5), int), dict(n_correct=7, n_total=7, objects=[(7, 7)]))
    t = np.ones((3, 3), np.int32)
    t[1, 1] = 0
    p = np.zeros((3, 3), int)
    p[1, 1] = 2
    q["frame_ring"] = (t, p, dict(n_correct=8, n_total=8, objects=[(8, 9)]))
    # a full map (class 1 everywhere, predicted class 1 on the left half of 4 x 6) and an empty map
    p = np.zeros((4, 6), int)
    p[:, 3:] = 1
    q["full_map"] = (np.ones((4, 6), np.int32), p, dict(n_correct=12, n_total=24, objects=[(12, 24)]))
    q["empty_map"] = (np.zeros((4, 6), np.int32), np.zeros((4, 6), int), dict(n_correct=0, n_total=0, objects=[]))
    return q


def logits_from_pred(pred, n_classes=3):
    """(h, w) predicted class -> (h, w, 1 + n_classes) float32 logits whose class argmax is pred (channel 0, the detection logit, is large: it must be ignored)"""
    h, w = pred.shape
    z = np.full((h, w, 1 + n_classes), -1.0, np.float32)
    z[..., 0] = 9.0
    np.put_along_axis(z, (np.asarray(pred) + 1)[..., None], 2.0, axis=-1)
    return z
