"""Geometric and photometric augmentation on the MI355X -- host mirror of semantic_segmentation/augmentation.py.

The reference augments every training image on the host with Pillow at full source resolution (augmentation.py:50-85): a
random rotation in +-45 degrees, a random crop that keeps all markup, a quarter turn (+-90 / 180 degrees), a random
perspective distortion, and an imgaug photometric stage.  Here the parameters are drawn on the host (``sample_plan``,
the reference's draws in the reference's order), every image size follows from them on the host, the markup is transformed
on the host in float64 (``apply_plan_to_markup``), and the pixels are warped on the device by ``ubd_warp_images``
(csrc/warp.hip), bit-identical to Pillow: at most two passes per image (rotation; perspective or a final copy) -- crops and
quarter turns are signed strided views that the next pass reads through.

The photometric (imgaug) stage (augmentation.py:83-84, :276-332: ``iaa.SomeOf((0, 5), [13 entries], random_order=True)``) runs
after the warps, on the device, when the caller hands ``sample_plan`` a generator for it (``photo_rng``; imgaug keeps its own
generator too): ``sample_photometric`` draws up to five stages, ``photometric_descs`` turns a stage into the integer descriptor
of ``ubd_photometric_images`` (csrc/photometric.hip), ``augment_arrays_on_device`` runs them slot by slot.  Built: GaussianBlur,
AverageBlur, Sharpen, Emboss, AdditiveGaussianNoise, Dropout, Invert, Add, Multiply, ContrastNormalization, Grayscale; and,
drawn only with ``extended=True`` / ``photo_extended=True`` (``PHOTO_EXTENDED``; off by default, so every earlier plan and
stream stays as it was): MedianBlur, AddToHueAndSaturation (the hue wraps; imgaug of the reference's era clips it) and
ElasticTransformation (cv2.remap's bicubic; imgaug of the reference's era uses a scipy spline).  Without the flag these three
are recorded as ``Stage("unbuilt", {"name": ...})`` and change no pixel.
The last two, drawn only with ``noise_alpha=True`` / ``photo_noise_alpha=True`` (``PHOTO_NOISE_ALPHA``; off by default too, and
independent of the other flag): SimplexNoiseAlpha(EdgeDetect / DirectedEdgeDetect) and FrequencyNoiseAlpha(Multiply,
ContrastNormalization).  Both blend two processed copies of the image by a smooth random mask: ``simplex_grid`` /
``frequency_grid`` make the mask's tiny noise grids on the host (at most 16 x 16 cells: ``noise_alpha_grid_size``),
``alpha_curve`` its sigmoid table, ``noise_alpha_descs`` lowers a stage to the descriptor of ``ubd_noise_alpha_images``
(csrc/noise_alpha.hip), which upscales, aggregates, applies the curve, makes both branches and blends in one kernel.  Without
the flag they too are recorded as ``unbuilt``.  With both flags no operation of the reference's stage is left out.
imgaug and OpenCV are not available to compare with: each built operation follows the libraries' published behaviour in integer
arithmetic DEFINED by include/ubd.h, tests/photometric_oracle.py, tests/photometric_ext_oracle.py and
tests/noise_alpha_oracle.py, which the device matches bit for bit; PARITY WITH imgaug / cv2 IS UNPINNED: the random stream is
numpy's, not imgaug's; the simplex generator is the classic 2-D simplex noise, not the OpenSimplex package imgaug calls; the
mask's grids are capped at 16 x 16 cells; cv2.resize's coefficients are restated at 1/32-pixel phases.
Without ``photo_rng`` the stage's decision draw is consumed, the plan records it (``photometric_requested``) and the pixels
are left as the geometric chain made them.
Flips have probability 0 in the reference: their draws are consumed, they are never applied.
"""
import collections
import ctypes
import logging
import math
import random as _random

import numpy as np
import torch
from PIL import Image

from . import _lib

# kind: 'rotate' {angle}, 'crop' {box: unrounded (left, top, right, bottom), window: Pillow's rounded (x0, y0, x1, y1)},
# 'quarter' {angle: 90 | -90 | 180}, 'perspective' {coeffs: 8 floats}; size: (w, h) after the stage
# photometric stages (size None; every params has 'entry', the index into PHOTO_ENTRIES; per-channel parameters are 3-tuples):
# 'gaussian_blur' {sigma}, 'average_blur' {k}, 'sharpen' {alpha, lightness}, 'emboss' {alpha, strength},
# 'noise' {scale, per_channel, seed}, 'dropout' {p, per_channel, seed}, 'invert' {channels}, 'add' {values, per_channel},
# 'multiply' {factors, per_channel}, 'contrast' {alphas, per_channel}, 'grayscale' {alpha}, 'unbuilt' {name};
# drawn only with extended=True: 'median_blur' {k}, 'hue_saturation' {value}, 'elastic' {applied, sigma; alpha, seed when applied}
# drawn only with noise_alpha=True: 'simplex_alpha' {directed, alpha, direction (directed only), + the mask parameters},
# 'frequency_alpha' {exponent, factors, contrast_alpha, + the mask parameters}; the mask parameters: iterations (a tuple of
# {size, upscale: 'nearest' | 'linear' | 'cubic', seed}), aggregation: 'max' | 'avg', sigmoid, threshold
Stage = collections.namedtuple("Stage", ["kind", "params", "size"])
# size: (w, h) of the source image; original: the 10 % "feed the original" branch was taken (no further draws);
# photometric_requested: the reference would have run its imgaug stage here; photometric: that stage's operations, drawn only
# when sample_plan is given a generator for them (module docstring)
AugmentationPlan = collections.namedtuple("AugmentationPlan", ["size", "stages", "original", "photometric_requested", "photometric"],
                                          defaults=[()])

FEED_ORIGINAL_P, ROTATE_P, CROP_P, HFLIP_P, VFLIP_P, ROTATE_90_P, PERSPECTIVE_P, PHOTOMETRIC_P = 0.1, 0.5, 0.5, 0, 0, 0.5, 0.5, 0.7
ROTATION_90_ANGLES = [90, -90, 180]
MAX_CROP_MARGIN = 0.4
PERSPECTIVE_MEAN = np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64)
PERSPECTIVE_HALF = np.array([0.1, 0.1, 50, 0.1, 0.1, 50, 0.0002, 0.0002], np.float64)


def identity_plan(size):
    return AugmentationPlan((int(size[0]), int(size[1])), (), False, False)


# ---------------------------------------------------------------------------------------------------------------- sizes
def rotate_matrix_and_size(angle, size):
    """What ``Image.rotate(angle, BILINEAR, expand=True)`` does with an image of ``size`` = (w, h) (Pillow's Image.py, restated):
    returns (kind, matrix, (new_w, new_h)) with kind 'copy' (angle % 360 == 0), 'quarter' (90 / 180 / 270: an exact
    ``Image.transpose``; matrix is the angle) or 'affine' (matrix: the six AFFINE coefficients, destination -> source)."""
    w, h = size
    angle = angle % 360.0
    if angle == 0:
        return "copy", None, (w, h)
    if angle == 180:
        return "quarter", 180, (w, h)
    if angle in (90, 270):
        return "quarter", int(angle), (h, w)
    center = (w / 2, h / 2)
    angle = -math.radians(angle)
    matrix = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
              round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y, matrix):
        a, b, c, d, e, f = matrix
        return a * x + b * y + c, d * x + e * y + f

    matrix[2], matrix[5] = transform(-center[0] - 0, -center[1] - 0, matrix)
    matrix[2] += center[0]
    matrix[5] += center[1]
    xx, yy = [], []
    for x, y in ((0, 0), (w, 0), (w, h), (0, h)):
        tx, ty = transform(x, y, matrix)
        xx.append(tx)
        yy.append(ty)
    nw = math.ceil(max(xx)) - math.floor(min(xx))
    nh = math.ceil(max(yy)) - math.floor(min(yy))
    matrix[2], matrix[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0, matrix)
    return "affine", matrix, (nw, nh)


def crop_window(box):
    """``Image.crop``'s integer window for a float box: Python's ``round`` (half to even) of every coordinate."""
    return tuple(int(round(v)) for v in box)


# --------------------------------------------------------------------------------------------------------------- markup
def _shapely_cos_sin(angle_degrees):
    """cosine and sine as shapely.affinity.rotate takes them: values below 2.5e-16 in magnitude are exactly zero, so quarter
    turns move integer markup to integers (12.000000000000002 would be ceiled to 13 by _proper_round)."""
    a = angle_degrees * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    return (0.0 if abs(c) < 2.5e-16 else c), (0.0 if abs(s) < 2.5e-16 else s)


def _rotate_points(pts, image_angle, size, new_size):
    """augmentation.py:165-176, :248-260: the image turns by ``image_angle`` (counter-clockwise on the screen), so the points
    turn by -image_angle in the y-down frame, about the old centre, and move to the new centre."""
    c, s = _shapely_cos_sin(-image_angle)
    x = pts[:, 0] - size[0] / 2
    y = pts[:, 1] - size[1] / 2
    return np.stack([c * x - s * y + new_size[0] / 2, s * x + c * y + new_size[1] / 2], axis=1)


def perspective_point_matrix(coeffs):
    """augmentation.py:203-208: Pillow's PERSPECTIVE data maps destination to source, so points move by the inverse 3x3"""
    return np.linalg.inv(np.reshape(list(coeffs) + [1], (3, 3)).astype(np.float64))


def _perspective_points(pts, coeffs):
    m = perspective_point_matrix(coeffs)
    res = np.vstack((pts.T, np.ones((1, pts.shape[0]))))
    res = np.dot(m, res)
    res /= res[-1, :]
    return res[:-1].T


def _stage_points(stage, pts, size):
    """(n, 2) float64 points of an image of ``size`` through one stage"""
    if stage.kind in ("rotate", "quarter"):
        return _rotate_points(pts, stage.params["angle"], size, stage.size)
    if stage.kind == "crop":
        left, top = stage.params["box"][0], stage.params["box"][1]
        return pts + np.array([[-left, -top]])
    if stage.kind == "perspective":
        return _perspective_points(pts, stage.params["coeffs"])
    raise ValueError(f"unknown stage kind {stage.kind!r}")


def _markup_points(markup):
    return [np.array(m.bbox, dtype=np.float64).reshape(-1, 2) for m in markup]


def apply_plan_to_markup(plan, markup):
    """The markup of an image after ``plan``: new objects of the same type (``create_same_markup``) around float64 boxes;
    the caller's objects are not touched.  Empty / None markup is returned as it is."""
    if not markup:
        return markup
    boxes = _markup_points(markup)
    size = plan.size
    for stage in plan.stages:
        boxes = [_stage_points(stage, b, size) for b in boxes]
        size = stage.size
    return [m.create_same_markup(b.reshape(-1)) for m, b in zip(markup, boxes)]


# -------------------------------------------------------------------------------------------------------------- sampler
def _normalize_rect(rect, image_size):
    """augmentation.py:126-162: the markup bounds clipped to the image and widened along one axis when their aspect is
    far from the image's.  Raises ZeroDivisionError for bounds of zero height."""
    r = list(rect)
    r[0] = max(0, r[0])
    r[1] = max(0, r[1])
    r[2] = min(image_size[0], r[2])
    r[3] = min(image_size[1], r[3])
    rect_width = r[2] - r[0]
    rect_height = r[3] - r[1]
    ratio = rect_width / rect_height
    image_ratio = image_size[0] / image_size[1]
    if ratio < image_ratio * 0.7:
        new_width = image_ratio * rect_height
        if r[0] < (image_size[0] - new_width) / 2:
            r[2] = r[0] + new_width
        elif r[2] > (image_size[0] + new_width) / 2:
            r[0] = r[2] - new_width
        else:
            r[0] = (image_size[0] - new_width) / 2
            r[2] = r[0] + new_width
    elif ratio > image_ratio * 1.3:
        new_height = rect_width / image_ratio
        if r[1] < (image_size[1] - new_height) / 2:
            r[3] = r[1] + new_height
        elif r[3] > (image_size[1] + new_height) / 2:
            r[1] = r[3] - new_height
        else:
            r[1] = (image_size[1] - new_height) / 2
            r[3] = r[1] + new_height
    return r


def _sample_crop(boxes, size, rng):
    """augmentation.py:94-117: the four draws of the crop (left, top, right, bottom).  Returns the stage, or None (nothing
    drawn) when the markup bounds have no width or no height."""
    allp = np.concatenate(boxes, axis=0)
    bounds = [float(allp[:, 0].min()), float(allp[:, 1].min()), float(allp[:, 0].max()), float(allp[:, 1].max())]
    if not (bounds[2] > bounds[0] and bounds[3] > bounds[1]):
        logging.warning("augmentation: markup bounds %s have no width or no height; crop skipped", bounds)
        return None
    try:
        rect = _normalize_rect(bounds, size)
    except ZeroDivisionError:
        logging.warning("augmentation: markup bounds %s have no height inside the %d x %d image; crop skipped", bounds, size[0], size[1])
        return None
    w, h = size
    max_left = min(MAX_CROP_MARGIN * w, rect[0])
    max_right = min(MAX_CROP_MARGIN * w, w - rect[2])
    max_top = min(MAX_CROP_MARGIN * h, rect[1])
    max_bottom = min(MAX_CROP_MARGIN * h, h - rect[3])
    left = rng.uniform(0, max_left)
    top = rng.uniform(0, max_top)
    right = w - rng.uniform(0, max_right)
    bottom = h - rng.uniform(0, max_bottom)
    box = (left, top, right, bottom)
    x0, y0, x1, y1 = crop_window(box)
    if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
        logging.warning("augmentation: crop box %s rounds to the window %s, which is empty or leaves the %d x %d image; crop skipped",
                        box, (x0, y0, x1, y1), w, h)
        return None
    return Stage("crop", {"box": box, "window": (x0, y0, x1, y1)}, (x1 - x0, y1 - y0))


def sample_plan(image_size, markup, rng=None, np_rng=None, photo_rng=None, photo_extended=False, photo_noise_alpha=False):
    """Draws the parameters of the reference's ``__augment_image`` (augmentation.py:50-85) for one image of ``image_size`` =
    (w, h) and its ``markup`` and returns an ``AugmentationPlan``: the stages with their numbers and the image size after each.

    The generators are consumed in the reference's order, so seeding ``random`` and ``numpy.random`` as augmentation.py:29-31
    invites gives the reference's parameter stream: nothing for empty markup; ``random()`` (< 0.1: feed the original, stop);
    ``random()`` (< 0.5) -> ``uniform(-45, 45)``; ``random()`` (< 0.5) -> four ``uniform`` (left, top, right, bottom);
    two ``random()`` for the flips (probability 0); ``random()`` (< 0.5) -> ``choice([90, -90, 180])`` and the
    ``uniform(angle, angle)`` of the reference's ``__rotate``; ``random()`` (< 0.5) -> one ``np_rng.uniform`` of 8 numbers;
    ``random()`` (< 0.7) for the photometric stage: the plan records that it was requested.
    ``rng`` / ``np_rng``: objects with the interface of the ``random`` / ``numpy.random`` modules (the defaults).
    ``photo_rng``: a ``numpy.random.Generator`` for the photometric stage's own draws (imgaug keeps its own generator too);
    when it is given and the stage was requested, ``plan.photometric = sample_photometric(3, photo_rng, photo_extended,
    photo_noise_alpha)`` (per-channel parameters for three channels; a grey image uses the first).  Nothing more is drawn from ``rng`` / ``np_rng`` either way.
    A stage whose input is degenerate (markup bounds without width or height, a crop that rounds to an empty window) is
    skipped with a warning and the chain goes on."""
    rng = _random if rng is None else rng
    np_rng = np.random if np_rng is None else np_rng
    size = (int(image_size[0]), int(image_size[1]))
    if markup is None or len(markup) == 0:
        return AugmentationPlan(size, (), False, False)
    if rng.random() < FEED_ORIGINAL_P:
        return AugmentationPlan(size, (), True, False)
    boxes = _markup_points(markup)
    stages = []
    cur = size

    def push(stage):
        nonlocal boxes, cur
        boxes = [_stage_points(stage, b, cur) for b in boxes]
        cur = stage.size
        stages.append(stage)

    if rng.random() < ROTATE_P:
        angle = rng.uniform(-45, 45)
        push(Stage("rotate", {"angle": angle}, rotate_matrix_and_size(angle, cur)[2]))
    if rng.random() < CROP_P:
        stage = _sample_crop(boxes, cur, rng)
        if stage is not None:
            push(stage)
    rng.random()                                        # horizontal flip, probability 0
    rng.random()                                        # vertical flip, probability 0
    if rng.random() < ROTATE_90_P:
        angle = rng.choice(ROTATION_90_ANGLES)
        angle = rng.uniform(angle, angle)               # the draw of the reference's __rotate; the value is `angle` exactly
        push(Stage("quarter", {"angle": int(angle)}, rotate_matrix_and_size(angle, cur)[2]))
    if rng.random() < PERSPECTIVE_P:
        coeffs = np_rng.uniform(PERSPECTIVE_MEAN - PERSPECTIVE_HALF, PERSPECTIVE_MEAN + PERSPECTIVE_HALF).tolist()
        push(Stage("perspective", {"coeffs": coeffs}, cur))
    photometric = rng.random() < PHOTOMETRIC_P
    if photometric and photo_rng is not None:
        return AugmentationPlan(size, tuple(stages), False, True, sample_photometric(3, photo_rng, photo_extended, photo_noise_alpha))
    return AugmentationPlan(size, tuple(stages), False, bool(photometric))


# ---------------------------------------------------------------------------------------------------------- photometric
# the 13 top-level entries of the reference's iaa.SomeOf (augmentation.py:290-327), in its list order
PHOTO_ENTRIES = ("blur", "sharpen", "emboss", "edge_detect", "noise", "dropout", "invert", "add", "hue_saturation", "multiply",
                 "contrast", "grayscale", "elastic")
PHOTO_UNBUILT = ("MedianBlur", "SimplexNoiseAlpha", "AddToHueAndSaturation", "FrequencyNoiseAlpha", "ElasticTransformation")
# the three of them that sample_photometric(..., extended=True) draws as stages of their own
PHOTO_EXTENDED = ("MedianBlur", "AddToHueAndSaturation", "ElasticTransformation")
# the other two, which sample_photometric(..., noise_alpha=True) draws as stages of their own
PHOTO_NOISE_ALPHA = ("SimplexNoiseAlpha", "FrequencyNoiseAlpha")
NOISE_ALPHA_KINDS = ("simplex_alpha", "frequency_alpha")
NOISE_ALPHA_MAX_GRID = 16             # cells per side of a mask grid: the limit of ubd_noise_alpha_images (imgaug has none)
PHOTO_POINTWISE = (_lib.UBD_PHOTO_AFFINE, _lib.UBD_PHOTO_GREY, _lib.UBD_PHOTO_NOISE, _lib.UBD_PHOTO_DROPOUT, _lib.UBD_PHOTO_HSV)
ELASTIC_SIGMA = 0.25


def sample_photometric(channels, gen, extended=False, noise_alpha=False):
    """The draws of the reference's imgaug stage (augmentation.py:280-330) from ``gen``, a ``numpy.random.Generator``: a tuple of
    ``Stage``s (``size`` None) in the order they are applied.  Order of the draws: ``n = gen.integers(0, 6)``;
    ``gen.permutation(13)[:n]`` over ``PHOTO_ENTRIES`` (SomeOf((0, 5)), random_order=True); per chosen entry its parameters in
    the order the reference lists them (a parameter that may be per channel: ``channels`` values), then the ``per_channel``
    coin (``gen.random() < 0.5``) where the reference has ``per_channel=0.5``, then a 64-bit seed for noise / dropout.  The blur
    entry first draws ``gen.integers(0, 3)`` (gaussian / average / median), the multiply entry ``gen.integers(0, 2)`` (Multiply /
    FrequencyNoiseAlpha), the elastic entry its ``sometimes`` coin.  A draw that lands on an operation that is not built
    (``PHOTO_UNBUILT``) gives ``Stage("unbuilt", {"name": ...}, None)``: recorded, no pixels change, so the built operations
    occur as often as in the reference.  The stream is numpy's, not imgaug's.
    ``extended``: the three operations of ``PHOTO_EXTENDED`` draw their parameters in place of the ``unbuilt`` stage -- MedianBlur
    ``k = gen.integers(3, 12)``, an even k becoming k + 1 (imgaug's rule); AddToHueAndSaturation one ``gen.integers(-20, 21)`` for
    both channels; ElasticTransformation, after its coin and only when applied, ``gen.uniform(0.5, 3.5)`` (alpha) and a 64-bit
    seed, sigma 0.25.  Every other entry, the count and the permutation draw as without it.
    ``noise_alpha``: independent of ``extended``; the two operations of ``PHOTO_NOISE_ALPHA`` draw their parameters in place of
    the ``unbuilt`` stage, in this order.  The edge_detect entry (``"simplex_alpha"``): ``gen.integers(0, 2)`` (EdgeDetect /
    DirectedEdgeDetect), alpha ``gen.uniform(0.5, 1.0)``, for the directed form direction ``gen.uniform(0, 1)``, then the mask.
    The FrequencyNoiseAlpha branch of the multiply entry (``"frequency_alpha"``): exponent ``gen.uniform(-4, 0)``, ``channels``
    Multiply factors ``gen.uniform(0.5, 1.5)`` (per_channel=True in the reference), one contrast alpha ``gen.uniform(0.5, 2.0)``,
    then the mask.  The mask: iterations ``gen.integers(1, 4)``; per iteration ``size_px_max = gen.integers(lo, 17)`` (lo = 2
    for simplex, 4 for frequency), the upscale method from one ``gen.random()`` (< 0.05 nearest, < 0.65 linear, else cubic)
    and a 64-bit seed; then, frequency only, aggregation ``gen.integers(0, 2)`` (0 avg, 1 max) and the
    sigmoid coin ``gen.random() < 0.5`` (simplex: max, sigmoid on); last the threshold ``gen.normal(0, 5)``."""
    c = int(channels)

    def per_channel(values):
        values = tuple(values)
        shared = not gen.random() < 0.5
        return (values[:1] * c if shared else values), not shared

    def seed():
        return int(gen.integers(0, 2 ** 64, dtype=np.uint64))

    def mask(lo):
        its = []
        for _ in range(int(gen.integers(1, 4))):
            size = int(gen.integers(lo, 17))
            r = float(gen.random())                                      # p = 0.05 / 0.6 / 0.35
            its.append({"size": size, "upscale": "nearest" if r < 0.05 else ("linear" if r < 0.65 else "cubic"), "seed": seed()})
        return tuple(its)

    n = int(gen.integers(0, 6))
    stages = []
    for e in gen.permutation(len(PHOTO_ENTRIES))[:n].tolist():
        name = PHOTO_ENTRIES[e]
        if name == "blur":
            which = int(gen.integers(0, 3))
            if which == 0:
                st = ("gaussian_blur", {"sigma": float(gen.uniform(0.0, 3.0))})
            elif which == 1:
                st = ("average_blur", {"k": int(gen.integers(2, 8))})
            elif extended:
                k = int(gen.integers(3, 12))
                st = ("median_blur", {"k": k + 1 - k % 2})
            else:
                st = ("unbuilt", {"name": "MedianBlur"})
        elif name == "sharpen":
            st = ("sharpen", {"alpha": float(gen.uniform(0.0, 1.0)), "lightness": float(gen.uniform(0.75, 1.5))})
        elif name == "emboss":
            st = ("emboss", {"alpha": float(gen.uniform(0.0, 1.0)), "strength": float(gen.uniform(0.0, 2.0))})
        elif name == "edge_detect":
            if noise_alpha:
                directed = bool(int(gen.integers(0, 2)))
                q = {"directed": directed, "alpha": float(gen.uniform(0.5, 1.0))}
                if directed:
                    q["direction"] = float(gen.uniform(0.0, 1.0))
                q.update(iterations=mask(2), aggregation="max", sigmoid=True, threshold=float(gen.normal(0.0, 5.0)))
                st = ("simplex_alpha", q)
            else:
                st = ("unbuilt", {"name": "SimplexNoiseAlpha"})
        elif name == "noise":
            scale = float(gen.uniform(0.0, 0.05 * 255))
            st = ("noise", {"scale": scale, "per_channel": bool(gen.random() < 0.5), "seed": seed()})
        elif name == "dropout":
            p = float(gen.uniform(0.01, 0.1))
            st = ("dropout", {"p": p, "per_channel": bool(gen.random() < 0.5), "seed": seed()})
        elif name == "invert":                                            # Invert(0.05, per_channel=True): one coin per channel
            st = ("invert", {"channels": tuple(bool(v) for v in gen.random(c) < 0.05)})
        elif name == "add":
            values, pc = per_channel(int(v) for v in gen.integers(-10, 11, size=c))
            st = ("add", {"values": values, "per_channel": pc})
        elif name == "hue_saturation":
            st = ("hue_saturation", {"value": int(gen.integers(-20, 21))}) if extended else ("unbuilt", {"name": "AddToHueAndSaturation"})
        elif name == "multiply":
            if int(gen.integers(0, 2)) == 0:
                factors, pc = per_channel(float(v) for v in gen.uniform(0.5, 1.5, size=c))
                st = ("multiply", {"factors": factors, "per_channel": pc})
            elif noise_alpha:
                q = {"exponent": float(gen.uniform(-4.0, 0.0)), "factors": tuple(float(v) for v in gen.uniform(0.5, 1.5, size=c)),
                     "contrast_alpha": float(gen.uniform(0.5, 2.0)), "iterations": mask(4)}
                q.update(aggregation=("avg", "max")[int(gen.integers(0, 2))], sigmoid=bool(gen.random() < 0.5),
                         threshold=float(gen.normal(0.0, 5.0)))
                st = ("frequency_alpha", q)
            else:
                st = ("unbuilt", {"name": "FrequencyNoiseAlpha"})
        elif name == "contrast":
            alphas, pc = per_channel(float(v) for v in gen.uniform(0.5, 2.0, size=c))
            st = ("contrast", {"alphas": alphas, "per_channel": pc})
        elif name == "grayscale":
            st = ("grayscale", {"alpha": float(gen.uniform(0.0, 1.0))})
        else:                                                             # sometimes(ElasticTransformation): Sometimes(0.5, ...)
            applied = bool(gen.random() < 0.5)
            if not extended:
                st = ("unbuilt", {"name": "ElasticTransformation", "applied": applied})
            elif applied:
                st = ("elastic", {"applied": True, "alpha": float(gen.uniform(0.5, 3.5)), "sigma": ELASTIC_SIGMA, "seed": seed()})
            else:
                st = ("elastic", {"applied": False, "sigma": ELASTIC_SIGMA})
        st[1]["entry"] = e
        stages.append(Stage(st[0], st[1], None))
    return tuple(stages)


def gaussian_taps(sigma):
    """(radius, Q14 weights at distance 0..radius) of GaussianBlur(sigma): kernel width max(5, int(3.3 sigma)), odd; the float64
    weights exp(-x^2 / 2 sigma^2) normalised, quantised to Q14, the centre adjusted so that all taps sum to 16384"""
    k = max(5, int(3.3 * sigma))
    k += 1 - k % 2
    r = k // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    wts = np.exp(-(x * x) / (2.0 * sigma * sigma))
    q = np.rint(wts / wts.sum() * 16384.0).astype(np.int64)
    q[r] += 16384 - int(q.sum())
    return r, [int(v) for v in q[r:]]


def elastic_taps(sigma):
    """(w0, w1): the Q14 taps of the 3-tap Gaussian that smooths ElasticTransformation's displacement field, w0 + 2 w1 = 16384.
    Radius 1 is scipy's ``int(4 sigma + 0.5)``; a sigma that needs a larger radius raises ValueError."""
    if not sigma > 0 or int(4.0 * sigma + 0.5) != 1:
        raise ValueError(f"elastic sigma {sigma} needs a filter radius other than 1; only the 3-tap field filter is built")
    g = math.exp(-1.0 / (2.0 * sigma * sigma))
    w1 = int(np.rint(16384.0 * g / (1.0 + 2.0 * g)))
    return 16384 - 2 * w1, w1


def _affine_p(ms, as_, c):
    """p[] of an AFFINE map for c channels: m_c then a_c in Q16, the unused channels the identity"""
    ms, as_ = list(ms)[:c], list(as_)[:c]
    return [int(v) for v in ms + [65536] * (3 - c) + as_ + [0] * (3 - c)]


def photometric_descs(stage, w, h, c):
    """The integer descriptor fields of one photometric stage for a w x h image of c channels (layout: ubd_photo_desc in
    include/ubd.h): {"mode", "flags", "seed", "p"} -- or None when the stage launches nothing: an unbuilt operation, Grayscale
    or AddToHueAndSaturation of a grey image, a blur with sigma < 1e-3, an ElasticTransformation whose coin said no.  The two
    mask-blended kinds (``NOISE_ALPHA_KINDS``) are no mode of that call: they RAISE ValueError here and are lowered by
    ``noise_alpha_descs`` (None would let a stage that changes pixels pass for one that launches nothing).  Pure host code."""
    kind, q = stage.kind, stage.params
    c = int(c)

    def desc(mode, p, flags=0, seed=0):
        return {"mode": mode, "flags": int(flags), "seed": int(seed), "p": [int(v) for v in p]}

    def affine(ms, as_):
        return desc(_lib.UBD_PHOTO_AFFINE, _affine_p(ms, as_, c))

    def filter3(alpha, e):
        k = (1.0 - alpha) * np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64) + alpha * np.array(e, np.float64)
        return desc(_lib.UBD_PHOTO_FILTER3, np.rint(k * 16384.0).astype(np.int64).reshape(-1))

    if kind == "unbuilt":
        return None
    if kind in NOISE_ALPHA_KINDS:
        raise ValueError(f"stage {kind!r} is no mode of ubd_photometric_images: lower it with noise_alpha_descs")
    if kind == "invert":
        return affine([-65536 if v else 65536 for v in q["channels"]], [255 * 65536 if v else 0 for v in q["channels"]])
    if kind == "add":
        return affine([65536] * 3, [int(v) * 65536 for v in q["values"]])
    if kind == "multiply":
        return affine([int(np.rint(f * 65536.0)) for f in q["factors"]], [0] * 3)
    if kind == "contrast":
        return affine([int(np.rint(a * 65536.0)) for a in q["alphas"]], [int(np.rint(128.0 * (1.0 - a) * 65536.0)) for a in q["alphas"]])
    if kind == "grayscale":
        return None if c == 1 else desc(_lib.UBD_PHOTO_GREY, [int(np.rint(q["alpha"] * 16384.0))])
    if kind == "sharpen":
        return filter3(q["alpha"], [[-1, -1, -1], [-1, 8 + q["lightness"], -1], [-1, -1, -1]])
    if kind == "emboss":
        s = q["strength"]
        return filter3(q["alpha"], [[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]])
    if kind == "gaussian_blur":
        if q["sigma"] < 1e-3:
            return None
        r, wts = gaussian_taps(q["sigma"])
        return desc(_lib.UBD_PHOTO_SEP, [r] + wts)
    if kind == "average_blur":
        return desc(_lib.UBD_PHOTO_BOX, [q["k"]])
    if kind == "noise":
        return desc(_lib.UBD_PHOTO_NOISE, [int(np.array([q["scale"]], np.float32).view(np.int32)[0])], q["per_channel"], q["seed"])
    if kind == "dropout":
        thr = int(math.floor(q["p"] * 4294967296.0))
        return desc(_lib.UBD_PHOTO_DROPOUT, [thr - (1 << 32) if thr >= (1 << 31) else thr], q["per_channel"], q["seed"])
    if kind == "median_blur":
        return desc(_lib.UBD_PHOTO_MEDIAN, [q["k"]])
    if kind == "hue_saturation":
        return None if c == 1 else desc(_lib.UBD_PHOTO_HSV, [q["value"], q["value"]])
    if kind == "elastic":
        if not q["applied"]:
            return None
        return desc(_lib.UBD_PHOTO_ELASTIC, [int(np.rint(256.0 * q["alpha"]))] + list(elastic_taps(q["sigma"])), seed=q["seed"])
    raise ValueError(f"unknown photometric stage kind {kind!r}")


# ---------------------------------------------------------------------------------------------------- mask-blended stages
def noise_alpha_grid_size(h, w, size_px_max):
    """(gh, gw): the coarse size of a mask grid for an h x w image (imgaug's ``size_px_max`` rule: the longer side becomes
    ``size_px_max``, the other keeps the aspect, at least 1; an image no larger than that keeps its size), both then clamped to
    ``NOISE_ALPHA_MAX_GRID`` = 16 -- that clamp exists only here: 16 x 16 is the largest grid ubd_noise_alpha_images takes."""
    h, w, s = int(h), int(w), int(size_px_max)
    if max(h, w) > s:
        gh, gw = max(1, h * s // max(h, w)), max(1, w * s // max(h, w))
    else:
        gh, gw = h, w
    return min(gh, NOISE_ALPHA_MAX_GRID), min(gw, NOISE_ALPHA_MAX_GRID)


def _quantise_grid(g):
    return np.clip(np.rint(32768.0 * g), 0, 32768).astype(np.uint16)


_SIMPLEX_GRAD = np.array([(1, 1), (-1, 1), (1, -1), (-1, -1), (1, 0), (-1, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (0, 1), (0, -1)], np.float64)


def simplex_grid(gh, gw, seed):
    """(gh, gw) uint16 in 0..32768 (Q15): classic 2-D simplex noise (Perlin 2001, in Gustavson's public-domain formulation,
    written from the algorithm) with the permutation table ``default_rng(seed).permutation(256)``, sampled at the integer
    coordinates (x, y) of the grid, n in [-1, 1] mapped to (n + 1) / 2 and quantised with rint(32768 g).  imgaug calls the
    OpenSimplex package instead: parity is unpinned."""
    perm = np.random.default_rng(seed).permutation(256)
    perm = np.concatenate([perm, perm, perm[:2]])
    f2, g2 = 0.5 * (math.sqrt(3.0) - 1.0), (3.0 - math.sqrt(3.0)) / 6.0
    yin, xin = np.mgrid[0:int(gh), 0:int(gw)].astype(np.float64)
    s = (xin + yin) * f2                                                  # skew to the simplex cell
    i, j = np.floor(xin + s), np.floor(yin + s)
    t = (i + j) * g2
    x0, y0 = xin - (i - t), yin - (j - t)                                 # distance from the cell origin
    i1 = (x0 > y0).astype(np.int64)                                       # lower triangle: (1, 0), upper: (0, 1)
    j1 = 1 - i1
    ii, jj = i.astype(np.int64) & 255, j.astype(np.int64) & 255
    n = np.zeros(xin.shape, np.float64)
    for di, dj, off in ((0, 0, 0.0), (i1, j1, g2), (1, 1, 2.0 * g2)):     # the three corners of the simplex
        x, y = x0 - di + off, y0 - dj + off
        grad = _SIMPLEX_GRAD[perm[ii + di + perm[jj + dj]] % 12]
        tt = 0.5 - x * x - y * y
        n += np.where(tt < 0, 0.0, tt ** 4 * (grad[..., 0] * x + grad[..., 1] * y))
    return _quantise_grid((70.0 * n + 1.0) / 2.0)


def frequency_grid(gh, gw, exponent, seed):
    """(gh, gw) uint16 in 0..32768 (Q15): imgaug's frequency noise.  ``R, A = default_rng(seed).random((2, gh, gw))``; the
    spectrum R f**exponent exp(2 pi i A) with f = sqrt(fx^2 + fy^2) from ``np.fft.fftfreq`` and the [0, 0] term 0; the real part
    of its inverse transform, min-max normalised to 0..1 (a constant field becomes 0.5), quantised with rint(32768 g)."""
    gh, gw = int(gh), int(gw)
    r, a = np.random.default_rng(seed).random((2, gh, gw))
    f = np.sqrt(np.fft.fftfreq(gh)[:, None] ** 2 + np.fft.fftfreq(gw)[None, :] ** 2)
    f[0, 0] = 1.0
    spectrum = r * f ** float(exponent) * np.exp(2j * np.pi * a)
    spectrum[0, 0] = 0.0
    g = np.real(np.fft.ifft2(spectrum))
    lo, hi = float(g.min()), float(g.max())
    g = (g - lo) / (hi - lo) if hi > lo else np.full(g.shape, 0.5)
    return _quantise_grid(g)


def alpha_curve(sigmoid, threshold):
    """257 uint16 in 0..16384 (Q14), the mask value at u = 128 i of Q15: with ``sigmoid`` imgaug's Sigmoid(mul=20, add=-10) moved by
    the threshold, T[i] = rint(16384 / (1 + exp(-(20 i / 256 - 10 - threshold)))) in float64; without, T[i] = 64 i."""
    i = np.arange(257, dtype=np.float64)
    if not sigmoid:
        return (64 * np.arange(257)).astype(np.uint16)
    return np.rint(16384.0 / (1.0 + np.exp(-(20.0 * i / 256.0 - 10.0 - float(threshold))))).astype(np.uint16)


EDGE_DETECT_KERNEL = ((0, 1, 0), (1, -4, 1), (0, 1, 0))


def directed_edge_kernel(direction):
    """imgaug's DirectedEdgeDetect matrix at alpha 1 for ``direction`` in 0..1 (a full turn): the direction vector at 360 d - 90
    degrees; each of the 8 neighbours gets (1 - angle between it and the vector / 180 degrees)^4; normalised to sum 1, negated,
    centre 1: the matrix sums to 0."""
    rad = math.radians(360.0 * float(direction)) - 0.5 * math.pi
    vec = np.array([math.cos(rad), math.sin(rad)])
    m = np.zeros((3, 3), np.float64)
    for y in (-1, 0, 1):
        for x in (-1, 0, 1):
            if (x, y) != (0, 0):
                cell = np.array([x, y], np.float64)
                ang = math.degrees(math.acos(float(np.clip(np.dot(cell / np.linalg.norm(cell), vec), -1.0, 1.0))))
                m[y + 1, x + 1] = (1.0 - ang / 180.0) ** 4
    m = -m / m.sum()
    m[1, 1] = 1.0
    return m


_NA_UPSCALE = {"nearest": _lib.UBD_NA_NEAREST, "linear": _lib.UBD_NA_LINEAR, "cubic": _lib.UBD_NA_CUBIC}


def noise_alpha_descs(stage, w, h, c):
    """One mask-blended stage (``NOISE_ALPHA_KINDS``) for a w x h image of c channels -> (fields, tables): the descriptor fields
    of ``ubd_noise_alpha_desc`` (include/ubd.h) -- {"first", "second": {"kind", "p"}, "grids": [{"gw", "gh", "upscale",
    "grid_offset"}], "aggregation", "curve_offset"} -- and the uint16 tables they point into, the grids then the curve (offsets
    count from the start of that array).  'simplex_alpha': first = FILTER3, the Q14 taps of (1 - alpha) identity + alpha E with E
    the EdgeDetect matrix or ``directed_edge_kernel``, lowered as Sharpen is; second = IDENTITY.  'frequency_alpha': first =
    AFFINE from the Multiply factors, second = AFFINE from the contrast alpha, with the formulas of ``photometric_descs``.  Pure
    host code."""
    kind, q = stage.kind, stage.params
    c = int(c)

    def affine(ms, as_):
        return {"kind": _lib.UBD_NA_AFFINE, "p": _affine_p(ms, as_, c)}

    if kind == "simplex_alpha":
        e = np.array(directed_edge_kernel(q["direction"]) if q["directed"] else EDGE_DETECT_KERNEL, np.float64)
        k = (1.0 - q["alpha"]) * np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64) + q["alpha"] * e
        first = {"kind": _lib.UBD_NA_FILTER3, "p": [int(v) for v in np.rint(k * 16384.0).astype(np.int64).reshape(-1)]}
        second = {"kind": _lib.UBD_NA_IDENTITY, "p": []}
    elif kind == "frequency_alpha":
        first = affine([int(np.rint(f * 65536.0)) for f in q["factors"]], [0] * 3)
        a = q["contrast_alpha"]
        second = affine([int(np.rint(a * 65536.0))] * 3, [int(np.rint(128.0 * (1.0 - a) * 65536.0))] * 3)
    else:
        raise ValueError(f"not a mask-blended stage: {kind!r}")
    grids, tables, pos = [], [], 0
    for it in q["iterations"]:
        gh, gw = noise_alpha_grid_size(h, w, it["size"])
        g = simplex_grid(gh, gw, it["seed"]) if kind == "simplex_alpha" else frequency_grid(gh, gw, q["exponent"], it["seed"])
        grids.append({"gw": gw, "gh": gh, "upscale": _NA_UPSCALE[it["upscale"]], "grid_offset": pos})
        tables.append(g.reshape(-1))
        pos += gh * gw
    tables.append(alpha_curve(q["sigmoid"], q["threshold"]))
    fields = {"first": first, "second": second, "grids": grids, "aggregation": _lib.UBD_NA_MAX if q["aggregation"] == "max" else _lib.UBD_NA_AVG,
              "curve_offset": pos}
    return fields, np.concatenate(tables).astype(np.uint16)


# --------------------------------------------------------------------------------------------------------------- device
WARP_DESC = np.dtype([("src_offset", np.int64), ("dst_offset", np.int64), ("src_xpitch", np.int32), ("src_ypitch", np.int32),
                      ("src_w", np.int32), ("src_h", np.int32), ("dst_w", np.int32), ("dst_h", np.int32), ("mode", np.int32),
                      ("reserved", np.int32), ("coeffs", np.float64, (8,))], align=True)      # ubd_warp_desc of include/ubd.h
PHOTO_DESC = np.dtype([("src_offset", np.int64), ("dst_offset", np.int64), ("w", np.int32), ("h", np.int32), ("mode", np.int32),
                       ("flags", np.int32), ("seed", np.uint64), ("p", np.int32, (24,))], align=True)   # ubd_photo_desc
_NA_BRANCH = np.dtype([("kind", np.int32), ("p", np.int32, (9,))], align=True)
_NA_GRID = np.dtype([("gw", np.int32), ("gh", np.int32), ("upscale", np.int32), ("reserved", np.int32), ("grid_offset", np.int64)], align=True)
NOISE_ALPHA_DESC = np.dtype([("src_offset", np.int64), ("dst_offset", np.int64), ("w", np.int32), ("h", np.int32), ("iterations", np.int32),
                             ("aggregation", np.int32), ("first", _NA_BRANCH), ("second", _NA_BRANCH), ("grid", _NA_GRID, (3,)),
                             ("curve_offset", np.int64)], align=True)                            # ubd_noise_alpha_desc, 192 bytes


class _View:
    """A signed strided view of an image in device memory: pixel (x, y) at ptr + x * xp + y * yp; ``keep`` holds the tensor alive"""
    __slots__ = ("ptr", "xp", "yp", "w", "h", "c", "keep")

    def __init__(self, ptr, w, h, c, keep):
        self.ptr, self.xp, self.yp, self.w, self.h, self.c, self.keep = int(ptr), c, w * c, int(w), int(h), c, keep

    def rebind(self, ptr, w, h, keep):
        """the view becomes the packed w x h image at ptr, kept alive by ``keep``"""
        self.__init__(ptr, w, h, self.c, keep)

    def packed(self):
        return self.xp == self.c and self.yp == self.w * self.c

    def crop(self, x0, y0, x1, y1):
        self.ptr += x0 * self.xp + y0 * self.yp
        self.w, self.h = x1 - x0, y1 - y0

    def quarter(self, angle):
        """Image.transpose(ROTATE_90 / ROTATE_180 / ROTATE_270): new(x, y) = old(w-1-y, x) / old(w-1-x, h-1-y) / old(y, h-1-x)"""
        angle = angle % 360
        if angle == 90:
            self.ptr += (self.w - 1) * self.xp
            self.xp, self.yp = self.yp, -self.xp
            self.w, self.h = self.h, self.w
        elif angle == 180:
            self.ptr += (self.w - 1) * self.xp + (self.h - 1) * self.yp
            self.xp, self.yp = -self.xp, -self.yp
        elif angle == 270:
            self.ptr += (self.h - 1) * self.yp
            self.xp, self.yp = -self.yp, self.xp
            self.w, self.h = self.h, self.w
        else:
            raise ValueError(f"not a quarter turn: {angle}")

    def span(self):
        ex, ey = (self.w - 1) * self.xp, (self.h - 1) * self.yp
        return self.ptr + min(ex, 0) + min(ey, 0), self.ptr + max(ex, 0) + max(ey, 0) + self.c


def _warp_pass(jobs, c, device):
    """One ubd_warp_images call: jobs = [(view, mode, coeffs, (dst_w, dst_h))]; the views are replaced by packed views of one
    new device buffer."""
    starts, pos = [], 0
    for _, _, _, (dw, dh) in jobs:
        starts.append(pos)
        pos += (dw * dh * c + 255) & ~255                     # every image on a 256-byte boundary: dword stores
    out = torch.empty(max(pos, 1), dtype=torch.uint8, device=device)
    spans = [v.span() for v, _, _, _ in jobs]
    base = min(lo for lo, _ in spans)
    src_bytes = max(hi for _, hi in spans) - base
    descs = np.zeros(len(jobs), WARP_DESC)
    for k, (v, mode, coeffs, (dw, dh)) in enumerate(jobs):
        d = descs[k]
        d["src_offset"], d["dst_offset"] = v.ptr - base, starts[k]
        d["src_xpitch"], d["src_ypitch"], d["src_w"], d["src_h"] = v.xp, v.yp, v.w, v.h
        d["dst_w"], d["dst_h"], d["mode"] = dw, dh, mode
        if coeffs is not None:
            d["coeffs"][:len(coeffs)] = coeffs
    _lib.launch("ubd_warp_images", device, ctypes.c_void_p(base), src_bytes, out.data_ptr(), out.numel(), descs.ctypes.data, c, len(jobs))
    for k, (v, _, _, (dw, dh)) in enumerate(jobs):
        v.rebind(out.data_ptr() + starts[k], dw, dh, out)


def warp_views_on_device(views, plans, device):
    """Runs the plans' pixel chains on the device, stage by stage over all images: pass 1 -- every rotation; crops and quarter
    turns only change the views; pass 2 -- every perspective, and a copy for images whose chain ends in a crop or a quarter
    turn.  Stream-ordered: no host synchronisation, no device-to-host copy.  The views end up packed."""
    c = views[0].c
    rest = []
    jobs = []
    for v, plan in zip(views, plans):
        if (v.w, v.h) != tuple(plan.size):
            raise ValueError(f"plan made for a {plan.size[0]} x {plan.size[1]} image, the image is {v.w} x {v.h}")
        stages = list(plan.stages)
        if stages and stages[0].kind == "rotate":
            kind, matrix, size = rotate_matrix_and_size(stages[0].params["angle"], (v.w, v.h))
            if kind == "affine":
                jobs.append((v, _lib.UBD_WARP_AFFINE, matrix, size))
                stages = stages[1:]
            elif kind == "copy":
                stages = stages[1:]
            else:
                stages[0] = Stage("quarter", {"angle": matrix}, size)
        rest.append(stages)
    if jobs:
        _warp_pass(jobs, c, device)
    jobs = []
    for v, stages in zip(views, rest):
        persp = None
        for st in stages:
            if st.kind == "crop":
                v.crop(*st.params["window"])
            elif st.kind == "quarter":
                v.quarter(st.params["angle"])
            elif st.kind == "perspective" and persp is None:
                persp = st.params["coeffs"]
            else:
                raise ValueError(f"stage {st.kind!r} out of the chain's order (rotate, crop, quarter, perspective)")
            if (v.w, v.h) != tuple(st.size):
                raise ValueError(f"plan says {st.size} after {st.kind}, the image is {(v.w, v.h)}")
        if persp is not None:
            jobs.append((v, _lib.UBD_WARP_PERSPECTIVE, persp, (v.w, v.h)))
        elif not v.packed():
            jobs.append((v, _lib.UBD_WARP_COPY, None, (v.w, v.h)))
    if jobs:
        _warp_pass(jobs, c, device)
    return views


def _photometric_pass(jobs, c, device):
    """One ubd_photometric_images call: jobs = [(view, descriptor fields, in_place)].  In-place images (pointwise modes on pixels
    this module owns) keep their views; the others are written to one new device buffer and their views replaced."""
    starts, pos = [], 0
    for v, _, in_place in jobs:
        starts.append(None if in_place else pos)
        if not in_place:
            pos += (v.w * v.h * c + 255) & ~255                   # every image on a 256-byte boundary: dword stores
    out = torch.empty(max(pos, 1), dtype=torch.uint8, device=device)
    size = [v.w * v.h * c for v, _, _ in jobs]
    dsts = [v.ptr if st is None else out.data_ptr() + st for (v, _, _), st in zip(jobs, starts)]
    src_base = min(v.ptr for v, _, _ in jobs)
    src_bytes = max(v.ptr + n for (v, _, _), n in zip(jobs, size)) - src_base
    dst_base = min(dsts)
    dst_bytes = max(d + n for d, n in zip(dsts, size)) - dst_base
    descs = np.zeros(len(jobs), PHOTO_DESC)
    for k, (v, f, _) in enumerate(jobs):
        d = descs[k]
        d["src_offset"], d["dst_offset"], d["w"], d["h"] = v.ptr - src_base, dsts[k] - dst_base, v.w, v.h
        d["mode"], d["flags"], d["seed"] = f["mode"], f["flags"], f["seed"]
        d["p"][:len(f["p"])] = f["p"]
    _lib.launch("ubd_photometric_images", device, ctypes.c_void_p(src_base), src_bytes, ctypes.c_void_p(dst_base), dst_bytes,
                descs.ctypes.data, c, len(jobs))
    for (v, _, _), st in zip(jobs, starts):
        if st is not None:
            v.rebind(out.data_ptr() + st, v.w, v.h, out)


def fill_noise_alpha_desc(d, f, table_base=0):
    """the fields of ``noise_alpha_descs`` into one element of a ``NOISE_ALPHA_DESC`` array, the table offsets moved by ``table_base``"""
    d["iterations"], d["aggregation"], d["curve_offset"] = len(f["grids"]), f["aggregation"], f["curve_offset"] + table_base
    for name in ("first", "second"):
        d[name]["kind"] = f[name]["kind"]
        d[name]["p"][:len(f[name]["p"])] = f[name]["p"]
    for k, g in enumerate(f["grids"]):
        d["grid"][k]["gw"], d["grid"][k]["gh"], d["grid"][k]["upscale"] = g["gw"], g["gh"], g["upscale"]
        d["grid"][k]["grid_offset"] = g["grid_offset"] + table_base


def _noise_alpha_pass(jobs, c, device):
    """One ubd_noise_alpha_images call: jobs = [(view, descriptor fields, tables)].  The jobs' tables travel as one array in one
    pinned, stream-ordered transfer; every image is written to one new device buffer and its view replaced."""
    starts, pos = [], 0
    for v, _, _ in jobs:
        starts.append(pos)
        pos += (v.w * v.h * c + 255) & ~255                       # every image on a 256-byte boundary: dword stores
    out = torch.empty(max(pos, 1), dtype=torch.uint8, device=device)
    size = [v.w * v.h * c for v, _, _ in jobs]
    src_base = min(v.ptr for v, _, _ in jobs)
    src_bytes = max(v.ptr + n for (v, _, _), n in zip(jobs, size)) - src_base
    descs = np.zeros(len(jobs), NOISE_ALPHA_DESC)
    table_base = 0
    for k, (v, f, tab) in enumerate(jobs):
        d = descs[k]
        d["src_offset"], d["dst_offset"], d["w"], d["h"] = v.ptr - src_base, starts[k], v.w, v.h
        fill_noise_alpha_desc(d, f, table_base)
        curve = tab[f["curve_offset"]:f["curve_offset"] + 257]
        # the device trusts the table values (include/ubd.h): grids are Q15 in 0..32768, the curve Q14 in 0..16384
        assert tab.dtype == np.uint16 and int(tab[:f["curve_offset"]].max(initial=0)) <= 32768 and int(curve.max()) <= 16384
        table_base += tab.size
    tables = np.concatenate([tab for _, _, tab in jobs])
    pinned = torch.empty(tables.size, dtype=torch.int16, pin_memory=True)
    pinned.numpy()[:] = tables.view(np.int16)
    dev_tables = pinned.to(device, non_blocking=True)             # stream-ordered; the pinned block is recycled in stream order
    _lib.launch("ubd_noise_alpha_images", device, ctypes.c_void_p(src_base), src_bytes, out.data_ptr(), out.numel(), descs.ctypes.data,
                dev_tables.data_ptr(), dev_tables.numel(), c, len(jobs))
    for (v, _, _), st in zip(jobs, starts):
        v.rebind(out.data_ptr() + st, v.w, v.h, out)


def photometric_views_on_device(views, plans, owned, device):
    """Runs ``plan.photometric`` of every image on its packed view, slot by slot: one ubd_photometric_images call per slot over
    the images that have a built stage there, and one ubd_noise_alpha_images call over those whose stage is a mask-blended one
    (``NOISE_ALPHA_KINDS``).  Pointwise stages run in place, neighbourhood stages (MEDIAN, ELASTIC and the mask-blended ones
    among them) go to a new buffer that is
    swapped in; a view whose pixels are not this module's (``owned[k]`` false: a caller's tensor that no warp pass copied) is
    never written: its first stage goes to a new buffer.  Stream-ordered, no host synchronisation."""
    c = views[0].c
    owned = list(owned)
    chains = [() if plan.original else tuple(plan.photometric) for plan in plans]
    for slot in range(max((len(ch) for ch in chains), default=0)):
        jobs, na_jobs = [], []
        for k, (v, ch) in enumerate(zip(views, chains)):
            if slot < len(ch) and ch[slot].kind in NOISE_ALPHA_KINDS:
                na_jobs.append((v,) + noise_alpha_descs(ch[slot], v.w, v.h, c))
                owned[k] = True
                continue
            f = photometric_descs(ch[slot], v.w, v.h, c) if slot < len(ch) else None
            if f is not None:
                jobs.append((v, f, owned[k] and f["mode"] in PHOTO_POINTWISE))
                owned[k] = True
        if jobs:
            _photometric_pass(jobs, c, device)
        if na_jobs:
            _noise_alpha_pass(na_jobs, c, device)
    return views


def _view_tensor(v):
    """the (h, w, c) uint8 tensor of a packed view"""
    off = v.ptr - v.keep.data_ptr()
    return v.keep.reshape(-1)[off:off + v.h * v.w * v.c].view(v.h, v.w, v.c)


def augment_arrays_on_device(arrays, plans, device=None):
    """(H, W, C) uint8 images (numpy arrays on the host, staged through one pinned buffer and one transfer, or tensors on the
    device, read in place and never written; all with the same C of 1 or 3) through their plans -> list of (h, w, C) uint8
    device tensors: the warp passes, then the photometric stages of ``plan.photometric`` (empty unless the plan was sampled with
    a ``photo_rng``; skipped for ``plan.original``), slot by slot.  An image without any pass is returned as a view of its
    source."""
    _lib.require_gpu("augmentation on the device")
    from .segmap_manager import _stage_host
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    if len(arrays) != len(plans):
        raise ValueError("one plan per image is required")
    if not arrays:
        return []
    c = int(arrays[0].shape[2])
    if c not in (1, 3) or any(a.ndim != 3 or a.shape[2] != c for a in arrays):
        raise ValueError("images must all be HxWx1 or all HxWx3")
    host = [k for k, a in enumerate(arrays) if not isinstance(a, torch.Tensor)]
    views = [None] * len(arrays)
    if host:
        staged, offs = _stage_host([arrays[k] for k in host], device)
        for k, off in zip(host, offs):
            views[k] = _View(staged.data_ptr() + int(off), arrays[k].shape[1], arrays[k].shape[0], c, staged)
    for k, a in enumerate(arrays):
        if views[k] is None:
            views[k] = _View(a.data_ptr(), a.shape[1], a.shape[0], c, a)
    warp_views_on_device(views, plans, device)
    owned = [not isinstance(a, torch.Tensor) or v.keep is not a for a, v in zip(arrays, views)]
    photometric_views_on_device(views, plans, owned, device)
    return [_view_tensor(v) for v in views]


class SegLinksImageAugmentation:
    """The reference's class (augmentation.py:34-91) for one PIL image ('L' or 'RGB') and its markup: draws a plan from the
    ``random`` / ``numpy.random`` modules (or the given generators), runs its geometric chain on the MI355X and returns a PIL
    image of the same mode.  Nothing is drawn and nothing changes for empty markup.  The caller's markup objects are not
    mutated.  The photometric (imgaug) stage runs only with ``photo_rng`` (a ``numpy.random.Generator``; module docstring: the
    built operations, those that ``photo_extended`` and ``photo_noise_alpha`` add, parity with imgaug / OpenCV unpinned); without it ``plan.photometric_requested`` says
    whether the reference would have run it.  Needs an MI355X (RuntimeError otherwise: no CPU fallback)."""

    def __init__(self, image, markup, net_config, rng=None, np_rng=None, plan=None, photo_rng=None, photo_extended=False,
                 photo_noise_alpha=False):
        _lib.require_gpu("SegLinksImageAugmentation")
        if image.mode not in ("L", "RGB"):
            raise ValueError(f"image mode must be 'L' or 'RGB', got {image.mode!r}")
        self.__net_config = net_config
        self.plan = sample_plan(image.size, markup, rng, np_rng, photo_rng, photo_extended, photo_noise_alpha) if plan is None else plan
        self.__aug_image, self.__aug_markup = image, markup
        if not self.plan.stages and (self.plan.original or not self.plan.photometric):
            return
        a = np.asarray(image)
        out = augment_arrays_on_device([np.ascontiguousarray(a[:, :, None] if a.ndim == 2 else a)], [self.plan])[0].cpu().numpy()
        self.__aug_image = Image.fromarray(out[:, :, 0] if image.mode == "L" else out, image.mode)
        self.__aug_markup = apply_plan_to_markup(self.plan, markup)

    def get_modified_image(self):
        return self.__aug_image

    def get_modified_markup(self):
        return self.__aug_markup
