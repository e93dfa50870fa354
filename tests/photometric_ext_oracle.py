"""Numpy definition of the three later modes of ubd_photometric_images (include/ubd.h, csrc/photometric.hip): MEDIAN (MedianBlur),
HSV (AddToHueAndSaturation) and ELASTIC (ElasticTransformation).

Like tests/photometric_oracle.py this file -- not imgaug or OpenCV, which are not available -- DEFINES the modes: each function
follows the libraries' published behaviour, restated in integer arithmetic with np.int64 from the descriptor's integer
parameters alone, and the device must equal it bit for bit.  Parity with imgaug / cv2 is unpinned.  Images are (h, w, c) uint8,
c = 1 or 3 (HSV: 3).  The product never imports this file.
"""
import numpy as np

from photometric_oracle import M32, philox4x32_10

MEDIAN, HSV, ELASTIC = 16, 17, 18


def median(img, k):
    """element (k k - 1) / 2 of the sorted k x k window, coordinates clamped to the edge (BORDER_REPLICATE), per channel"""
    h, w = img.shape[:2]
    r = k // 2
    ys = np.clip(np.arange(-r, h + r), 0, h - 1)
    xs = np.clip(np.arange(-r, w + r), 0, w - 1)
    pad = img[ys][:, xs]
    win = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)], axis=0)
    return np.sort(win, axis=0)[(k * k - 1) // 2]


def _recip(num, i):
    """(num + i) / (2 i) for i >= 1, 0 for i = 0"""
    i = np.asarray(i, dtype=np.int64)
    return np.where(i > 0, (num + i) // (2 * np.maximum(i, 1)), 0)


def hsv_forward(img):
    """(H 0..179, S, V) int64 of OpenCV's 8-bit RGB -> HSV with its Q12 reciprocal tables"""
    v = img.astype(np.int64)
    R, G, B = v[..., 0], v[..., 1], v[..., 2]
    V = np.maximum(np.maximum(R, G), B)
    D = V - np.minimum(np.minimum(R, G), B)
    S = (D * _recip(2088960, V) + 2048) >> 12
    hn = np.where(V == R, G - B, np.where(V == G, B - R + 2 * D, R - G + 4 * D))
    H = (hn * _recip(245760, D) + 2048) >> 12
    H = np.where(H < 0, H + 180, H)
    return H, S, V


def hsv_backward(H, S, V):
    """(h, w, 3) uint8 from H 0..179, S 0..255, V 0..255 (int64): sector i = H / 30, f = H - 30 i"""
    i = H // 30
    f = H - 30 * i
    P = (30 * V * (255 - S) + 3825) // 7650
    Q = (V * (7650 - S * f) + 3825) // 7650
    T = (V * (7650 - S * (30 - f)) + 3825) // 7650
    table = ((V, T, P), (Q, V, P), (P, V, T), (P, Q, V), (T, P, V), (V, P, Q))
    out = [np.select([i == s for s in range(6)], [table[s][ch] for s in range(6)]) for ch in range(3)]
    return np.stack(out, axis=-1).astype(np.uint8)


def hsv(img, dh, ds):
    if img.shape[2] != 3:
        raise ValueError("HSV needs three channels")
    H, S, V = hsv_forward(img)
    return hsv_backward(np.mod(H + int(dh), 180), np.clip(S + int(ds), 0, 255), V)


def elastic_field(h, w, w0, w1, seed):
    """(sx, sy): the smoothed Q15 field, int64 (h, w) each"""
    idx = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    zero = np.zeros_like(idx)
    r = philox4x32_10(np.stack([idx, zero, zero, zero], axis=-1), (int(seed) & M32, (int(seed) >> 32) & M32)).astype(np.int64)
    out = []
    for e in ((r[..., 0] >> 16) - 32768, (r[..., 1] >> 16) - 32768):
        p = np.pad(e, ((0, 0), (1, 1)))                                  # zero outside the image
        t = (w1 * p[:, :-2] + w0 * p[:, 1:-1] + w1 * p[:, 2:] + 8192) >> 14
        p = np.pad(t, ((1, 1), (0, 0)))
        out.append((w1 * p[:-2] + w0 * p[1:-1] + w1 * p[2:] + 8192) >> 14)
    return out[0], out[1]


def keys_weights(k):
    """the four Q17 weights of Keys' bicubic (a = -3/4) at phase k / 32, k any int64 array: (..., 4)"""
    k = np.asarray(k, dtype=np.int64)
    u = 32 - k
    return np.stack([-3 * k * u * u, 5 * k ** 3 - 288 * k * k + 131072, 5 * u ** 3 - 288 * u * u + 131072, -3 * u * k * k], axis=-1)


def elastic_positions(h, w, aq, w0, w1, seed):
    """(X, Y): the source position of every output pixel in 1 / 32 pixel"""
    sx, sy = elastic_field(h, w, int(w0), int(w1), seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    return 32 * xx + ((int(aq) * sx + (1 << 17)) >> 18), 32 * yy + ((int(aq) * sy + (1 << 17)) >> 18)


def elastic(img, aq, w0, w1, seed):
    h, w, c = img.shape
    X, Y = elastic_positions(h, w, aq, w0, w1, seed)
    ix, iy = X >> 5, Y >> 5
    wx, wy = keys_weights(X & 31), keys_weights(Y & 31)
    v = img.astype(np.int64)
    acc = np.zeros((h, w, c), np.int64)
    for j in range(4):
        yy = iy - 1 + j
        oky = (yy >= 0) & (yy < h)
        inner = np.zeros((h, w, c), np.int64)
        for i in range(4):
            xx = ix - 1 + i
            ok = oky & (xx >= 0) & (xx < w)
            tap = v[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]     # a tap outside the image contributes 0
            inner += wx[..., i, None] * tap
        acc += wy[..., j, None] * inner
    return np.clip((acc + (1 << 33)) >> 34, 0, 255).astype(np.uint8)


def apply(img, mode, p, flags=0, seed=0):
    """one stage from the descriptor's integer fields p[] (layout of include/ubd.h), modes 16..18"""
    p = [int(v) for v in p]
    if mode == MEDIAN:
        return median(img, p[0])
    if mode == HSV:
        return hsv(img, p[0], p[1])
    if mode == ELASTIC:
        return elastic(img, p[0], p[1], p[2], seed)
    raise ValueError(mode)
