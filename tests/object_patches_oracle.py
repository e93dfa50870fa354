"""Numpy restatement of ubd_extract_objects (include/ubd.h), written from its specification and not from the kernel: rescale,
orientation, expansion, Pillow's QUAD data, Pillow's quad_transform and bilinear filter.  All floating point is float64 with every
product and sum rounded on its own (numpy never fuses them); the integer steps use Python integers, which are exact.
tests/test_object_patches_host.py pins ``quad_data`` + ``sample`` against the installed Pillow bit for bit; the device is compared
with ``extract`` by tests/test_gpu_object_patches.py."""
import numpy as np

LIMIT = 2.0 ** 30


def rescale(quad, xscale=None, yscale=None):
    """8 integers -> [(X, Y)] * 4 Python integers: X = trunc(clamp(x * xscale, -2^30, 2^30)), toward zero; no scales: as they are."""
    pts = [(int(quad[2 * k]), int(quad[2 * k + 1])) for k in range(4)]
    if xscale is None:
        return pts

    def one(v, s):
        p = float(v) * float(s)
        return int(min(max(p, -LIMIT), LIMIT))           # int() truncates toward zero

    return [(one(x, xscale), one(y, yscale)) for x, y in pts]


def orient(pts):
    """[(X, Y)] * 4 integers -> (NW, NE, SE, SW): clockwise on the screen (y down), starting so that NW -> NE is a long side."""
    a2 = sum(pts[k][0] * pts[(k + 1) % 4][1] - pts[(k + 1) % 4][0] * pts[k][1] for k in range(4))
    c = [pts[0], pts[3], pts[2], pts[1]] if a2 < 0 else list(pts)
    e01 = (c[1][0] - c[0][0]) ** 2 + (c[1][1] - c[0][1]) ** 2
    e12 = (c[2][0] - c[1][0]) ** 2 + (c[2][1] - c[1][1]) ** 2
    r = 0 if e01 >= e12 else 1
    return [c[(r + k) % 4] for k in range(4)]


def expand_corners(corners, expand):
    """(NW, NE, SE, SW) integers -> float corners scaled by ``expand`` about the mean of the four; expand == 1.0: unchanged."""
    if expand == 1.0:
        return [(float(x), float(y)) for x, y in corners]
    cx = float((corners[0][0] + corners[1][0]) + (corners[2][0] + corners[3][0])) * 0.25
    cy = float((corners[0][1] + corners[1][1]) + (corners[2][1] + corners[3][1])) * 0.25
    return [(cx + (float(x) - cx) * expand, cy + (float(y) - cy) * expand) for x, y in corners]


def quad_data(corners, patch_w, patch_h):
    """float (NW, NE, SE, SW) -> the eight coefficients Image.__transformer hands to quad_transform for an output patch_w x patch_h"""
    nw, ne, se, sw = corners
    As, At = 1.0 / patch_w, 1.0 / patch_h
    out = []
    for d in (0, 1):
        out += [nw[d], (ne[d] - nw[d]) * As, (sw[d] - nw[d]) * At, ((((se[d] - sw[d]) - ne[d]) + nw[d]) * As) * At]
    return out


def sample(image, a, patch_w, patch_h):
    """(h, w, c) uint8 image, QUAD coefficients -> (patch_h, patch_w, c) uint8: quad_transform + the bilinear filter of 8-bit images"""
    image = np.asarray(image)
    h, w, c = image.shape
    out = np.zeros((patch_h, patch_w, c), np.uint8)
    if h == 0 or w == 0:
        return out
    xin = (np.arange(patch_w, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(patch_h, dtype=np.float64) + 0.5)[:, None]
    sx = ((a[0] + a[1] * xin) + a[2] * yin) + (a[3] * xin) * yin
    sy = ((a[4] + a[5] * xin) + a[6] * yin) + (a[7] * xin) * yin
    inside = (sx >= 0.0) & (sx < w) & (sy >= 0.0) & (sy < h)           # a NaN is outside
    sx = np.where(inside, sx, 0.5) - 0.5
    sy = np.where(inside, sy, 0.5) - 0.5
    xi, yi = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    dx, dy = sx - xi, sy - yi
    x0, x1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    yc = np.clip(yi, 0, h - 1)
    second = (yi + 1 >= 0) & (yi + 1 < h)
    y1 = np.where(second, yi + 1, yc)
    img = image.astype(np.int64)
    for ch in range(c):
        p00, p01, p10, p11 = img[yc, x0, ch], img[yc, x1, ch], img[y1, x0, ch], img[y1, x1, ch]
        v1 = p00 + (p01 - p00) * dx
        v2 = np.where(second, p10 + (p11 - p10) * dx, v1)
        v = v1 + (v2 - v1) * dy
        out[:, :, ch] = np.where(inside, v.astype(np.int64), 0).astype(np.uint8)     # truncation
    return out


def extract(image, quad, patch_h, patch_w, scales=None, expand=1.0):
    """One object: (patch (patch_h, patch_w, c) uint8, the 8 integers NW, NE, SE, SW of patch_quads)"""
    xs, ys = (None, None) if scales is None else scales
    corners = orient(rescale(quad, xs, ys))
    patch = sample(image, quad_data(expand_corners(corners, float(expand)), patch_w, patch_h), patch_w, patch_h)
    return patch, [v for p in corners for v in p]
