"""Numpy definition of ubd_noise_alpha_images (include/ubd.h, csrc/noise_alpha.hip): two processed copies of an image blended per
pixel by an upscaled, aggregated noise mask pushed through a curve.

Written from the definition in include/ubd.h, in np.int64 throughout, not from the kernel: the upscale is the plain double sum
over both axes' taps.  The branch results come from tests/photometric_oracle.py (FILTER3 / AFFINE).  The device must equal
``apply`` bit for bit.  Parity with imgaug / cv2 is unpinned.  Images are (h, w, c) uint8, c = 1 or 3; grids are (gh, gw) integer
arrays in 0..32768; the curve is 257 integers in 0..16384.  The product never imports this file.
"""
import numpy as np

import photometric_oracle as po

IDENTITY, FILTER3, AFFINE = range(3)
NEAREST, LINEAR, CUBIC = range(3)
MAX, AVG = range(2)


def keys_weights(k):
    """(..., 4) int64: the Q17 Keys weights (a = -3/4) at phase k / 32; they sum to 131072"""
    k = np.asarray(k, dtype=np.int64)
    u = 32 - k
    return np.stack([-3 * k * u * u, 5 * k ** 3 - 288 * k * k + 131072, 5 * u ** 3 - 288 * u * u + 131072, -3 * u * k * k], axis=-1)


def axis_taps(n, gn, up):
    """(index (n, T), weight (n, T)) int64 of every coordinate 0..n-1 of an axis of n pixels over gn cells"""
    x = np.arange(n, dtype=np.int64)
    if up == NEAREST:
        return np.minimum(gn - 1, (x * gn) // n)[:, None], np.ones((n, 1), np.int64)
    X = (2 * x + 1) * gn - n
    i = np.floor_divide(X, 2 * n)                                         # a true floor: X may be negative
    r = X - i * 2 * n
    k = (32 * r) // (2 * n)
    assert ((r >= 0) & (r < 2 * n) & (k >= 0) & (k <= 31)).all()
    if up == LINEAR:
        idx, wgt = np.stack([i, i + 1], axis=-1), np.stack([32 - k, k], axis=-1)
    else:
        idx, wgt = i[:, None] + np.arange(-1, 3)[None, :], keys_weights(k)
    return np.clip(idx, 0, gn - 1), wgt


def upscale(g, h, w, up):
    """(h, w) int64 in 0..32768: grid g to the image, the full double sum rounded once"""
    g = np.asarray(g, dtype=np.int64)
    iy, wy = axis_taps(h, g.shape[0], up)
    ix, wx = axis_taps(w, g.shape[1], up)
    s = np.zeros((h, w), np.int64)
    for j in range(iy.shape[1]):
        for i in range(ix.shape[1]):
            s += wy[:, j, None] * wx[None, :, i] * g[iy[:, j, None], ix[None, :, i]]
    if up == NEAREST:
        return s
    if up == LINEAR:
        return (s + 512) >> 10
    assert np.abs(s).max() < 2 ** 51
    return np.clip((s + 2 ** 33) >> 34, 0, 32768)


def mask(grids, h, w, aggregation, curve):
    """(h, w) int64 in 0..16384; grids: [(g, upscale)]"""
    us = [upscale(g, h, w, up) for g, up in grids]
    u = np.maximum.reduce(us) if aggregation == MAX else (np.sum(us, axis=0) + len(us) // 2) // len(us)
    t = np.asarray(curve, dtype=np.int64)
    assert t.shape == (257,)
    i, f = u >> 7, u & 127
    return np.where(f == 0, t[i], (t[i] * (128 - f) + t[np.minimum(i + 1, 256)] * f + 64) >> 7)


def branch(img, kind, p):
    if kind == IDENTITY:
        return img.copy()
    if kind == FILTER3:
        return po.apply(img, po.FILTER3, list(p)[:9])
    if kind == AFFINE:
        return po.apply(img, po.AFFINE, list(p)[:6])
    raise ValueError(kind)


def apply(img, first, second, grids, aggregation, curve):
    """first, second: (kind, p); grids: [(g, upscale)], 1..3 of them"""
    a = mask(grids, img.shape[0], img.shape[1], aggregation, curve)[..., None]
    f, s = branch(img, *first).astype(np.int64), branch(img, *second).astype(np.int64)
    return ((a * f + (16384 - a) * s + 8192) >> 14).astype(np.uint8)


def apply_fields(img, fields, tables):
    """the (fields, tables) of ubdvss_amd.augmentation.noise_alpha_descs"""
    grids = [(tables[g["grid_offset"]:g["grid_offset"] + g["gh"] * g["gw"]].reshape(g["gh"], g["gw"]), g["upscale"]) for g in fields["grids"]]
    curve = tables[fields["curve_offset"]:fields["curve_offset"] + 257]
    return apply(img, (fields["first"]["kind"], fields["first"]["p"]), (fields["second"]["kind"], fields["second"]["p"]), grids,
                 fields["aggregation"], curve)
