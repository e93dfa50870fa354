"""Numpy definition of the photometric augmentation modes of ubd_photometric_images (include/ubd.h, csrc/photometric.hip).

imgaug and OpenCV are not available, so this file -- not imgaug -- DEFINES the stage: every function follows imgaug's
published formula, restated in integer arithmetic, per pixel with np.int64, from the documented integer parameters alone.  The
device must equal these functions bit for bit (NOISE: up to the margin its fp32 transcendentals need).  Parity with imgaug /
cv2 is unpinned.  Images are (h, w, c) uint8, c = 1 or 3.  The product never imports this file.
"""
import numpy as np

AFFINE, GREY, FILTER3, SEP, BOX, NOISE, DROPOUT = range(7)
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32-valued, key: two uint32 values -> (..., 4) uint32 words"""
    c = [np.asarray(counter[..., k], dtype=np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                     # 32 x 32 -> 64 bits, exact in uint64
        c = [((p1 >> sh) ^ c[1] ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> sh) ^ c[3] ^ np.uint64(k1)) & mask, p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def pixel_words(h, w, seed):
    """(h, w, 8) uint32: r0..r7 of every pixel; key = seed (lo, hi), counter = (y w + x, 0, j, 0), j = 0, 1"""
    idx = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    key = (int(seed) & M32, (int(seed) >> 32) & M32)
    out = []
    for j in (0, 1):
        ctr = np.stack([idx, np.zeros_like(idx), np.full_like(idx, j), np.zeros_like(idx)], axis=-1)
        out.append(philox4x32_10(ctr, key))
    return np.concatenate(out, axis=-1)


def reflect101(i, n):
    """index i (any integer array) folded into 0..n-1 with period 2(n-1); always 0 for n = 1"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def _shifted(img, dy, dx):
    """img[reflect(y + dy), reflect(x + dx)] as int64"""
    h, w = img.shape[:2]
    return img.astype(np.int64)[reflect101(np.arange(h) + dy, h)][:, reflect101(np.arange(w) + dx, w)]


def _clamp(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def affine(img, m, a):
    """m, a: per channel int Q16"""
    c = img.shape[2]
    m = np.asarray(m, dtype=np.int64)[:c]
    a = np.asarray(a, dtype=np.int64)[:c]
    return _clamp((m * img.astype(np.int64) + a + 32768) >> 16)


def grey(img, aq):
    if img.shape[2] == 1:
        return img.copy()
    v = img.astype(np.int64)
    g = (4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14
    return (((16384 - aq) * v + aq * g[..., None] + 8192) >> 14).astype(np.uint8)


def filter3(img, taps):
    """taps: 9 int Q14, row-major; correlation"""
    acc = np.zeros(img.shape, np.int64)
    for dy in range(3):
        for dx in range(3):
            acc += int(taps[dy * 3 + dx]) * _shifted(img, dy - 1, dx - 1)
    return _clamp((acc + 8192) >> 14)


def sep(img, radius, weights):
    """weights[d]: Q14 weight at distance d = 0..radius"""
    t = np.zeros(img.shape, np.int64)
    for d in range(-radius, radius + 1):
        t += int(weights[abs(d)]) * _shifted(img, 0, d)
    t = (t + 64) >> 7
    h = img.shape[0]
    acc = np.zeros(img.shape, np.int64)
    for d in range(-radius, radius + 1):
        acc += int(weights[abs(d)]) * t[reflect101(np.arange(h) + d, h)]
    return _clamp((acc + (1 << 20)) >> 21)


def box(img, k):
    s = np.zeros(img.shape, np.int64)
    for dy in range(-(k // 2), k - (k // 2)):
        for dx in range(-(k // 2), k - (k // 2)):
            s += _shifted(img, dy, dx)
    return ((2 * s + k * k) // (2 * k * k)).astype(np.uint8)


def dropout(img, thr, per_channel, seed):
    h, w, c = img.shape
    r = pixel_words(h, w, seed)
    words = r[..., :c] if per_channel else np.repeat(r[..., :1], c, axis=-1)
    return np.where(words.astype(np.uint64) < np.uint64(thr), 0, img).astype(np.uint8)


def noise(img, scale, per_channel, seed):
    """scale: the fp32 value of the descriptor.  Returns (rounded uint8 image, unrounded float64 value v + scale z): z is
    computed in float64 from the same words, so the device's fp32 result may differ where the unrounded value is near a half"""
    h, w, c = img.shape
    r = pixel_words(h, w, seed).astype(np.uint64)
    z = np.empty((h, w, c), np.float64)
    for ch in range(c):
        a, b = (r[..., 2 * ch], r[..., 2 * ch + 1]) if per_channel else (r[..., 0], r[..., 1])
        u1 = ((a >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        u2 = ((b >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        z[..., ch] = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    exact = img.astype(np.float64) + float(np.float32(scale)) * z
    return _clamp(np.rint(exact)), exact


def apply(img, mode, p, flags=0, seed=0):
    """one stage from the descriptor's integer fields p[] (layout of include/ubd.h); NOISE returns the rounded image only"""
    p = [int(v) for v in p]
    if mode == AFFINE:
        return affine(img, p[0:3], p[3:6])
    if mode == GREY:
        return grey(img, p[0])
    if mode == FILTER3:
        return filter3(img, p[0:9])
    if mode == SEP:
        return sep(img, p[0], p[1:2 + p[0]])
    if mode == BOX:
        return box(img, p[0])
    if mode == NOISE:
        return noise(img, np.array([p[0]], np.int32).view(np.float32)[0], flags & 1, seed)[0]
    if mode == DROPOUT:
        return dropout(img, p[0] & M32, flags & 1, seed)
    raise ValueError(mode)


# ---- cases shared by tests/test_photometric_host.py and tests/test_gpu_photometric.py
NOISE_SHAPES = ((67, 130, 3), (9, 8, 1))                              # (h, w, c)
NOISE_SCALES = (0.0, 0.5, 12.75)


def make_image(rng, h, w, c, checker=None):
    """random pixels, or a +-255 pixel checkerboard with a per-channel phase"""
    if rng.random() < 0.35 if checker is None else checker:
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([((yy + xx + k) % 2) * 255 for k in range(c)], -1).astype(np.uint8)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def noise_cases():
    """(image, scale, per_channel, seed) of the NOISE checks.  On the 72-pixel image one pixel is 1.4 %: the generator seed is one
    for which the oracle has no pixel of that image within the margin (test_photometric_host.py asserts the shares)"""
    rng = np.random.default_rng(32)
    out = []
    for h, w, c in NOISE_SHAPES:
        for scale in NOISE_SCALES:
            for pc in (0, 1):
                out.append((make_image(rng, h, w, c, checker=False), scale, pc, int(rng.integers(0, 2 ** 64, dtype=np.uint64))))
    return out


def noise_margin(scale):
    return 1e-4 * (1.0 + scale)


def noise_excused(exact, scale):
    """pixels whose unrounded value lies within the margin of a half-integer"""
    return np.abs(exact - np.floor(exact) - 0.5) < noise_margin(scale)
