"""Test inputs of the Data Matrix decoder: an ECC 200 encoder for the square sizes 10 x 10 to 26 x 26 with tables of its own (the
field from its polynomial, the generator from its roots, the placement as a module map, the pad rule), written independently of
tests/matrix_decode_oracle.py, and a renderer that draws a symbol centred in a patch: supersampled four times, rotated with
bicubic resampling, brought down with a box filter, and optionally degraded (blur, an illumination ramp, noise)."""
import functools

import numpy as np

from decode_cases import _blur, _tint

SIZES = (10, 12, 14, 16, 18, 20, 22, 24, 26)
CAPACITY = {10: (3, 5), 12: (5, 7), 14: (8, 10), 16: (12, 12), 18: (18, 14), 20: (22, 18), 22: (30, 20), 24: (36, 24), 26: (44, 28)}
FNC1, PAD, UPPER_SHIFT = 232, 129, 235
DARK, LIGHT = 30.0, 220.0
DEGRADED = dict(blur=0.7, ramp=0.25, noise=5.0)


# --- GF(256), x^8 + x^5 + x^3 + x^2 + 1 (0x12D) ---------------------------------------
def gf_mul(a, b):
    """the product in GF(256) by shift and add: no table"""
    out = 0
    while b:
        if b & 1:
            out ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x12D
        b >>= 1
    return out


@functools.lru_cache(None)
def generator(e):
    """the coefficients of (x + a^1)(x + a^2)..(x + a^e), the highest power first (the leading 1 included)"""
    g, root = [1], 1
    for _ in range(e):
        root = gf_mul(root, 2)
        g = [x ^ y for x, y in zip(g + [0], [0] + [gf_mul(c, root) for c in g])]
    return tuple(g)


def check_codewords(data, e):
    """the e check codewords of the data codewords: the remainder of data(x) x^e by the generator"""
    g = generator(e)
    rem = [0] * e
    for d in data:
        f = d ^ rem[0]
        rem = [r ^ gf_mul(f, c) for r, c in zip(rem[1:] + [0], g[1:])]
    return rem


# --- codewords ------------------------------------------------------------------------
def codewords(text, gs1=False):
    """the ASCII encodation of ``text`` (a str of Latin-1 characters): a pair of digits is one codeword, a character of 128 and
    up takes the upper shift; gs1: FNC1 goes first and every '\\x1d' of the text is a FNC1"""
    out, k = [FNC1] if gs1 else [], 0
    while k < len(text):
        if text[k:k + 2].isdigit() and len(text[k:k + 2]) == 2 and text[k:k + 2].isascii():
            out.append(130 + int(text[k:k + 2]))
            k += 2
            continue
        v = ord(text[k])
        assert v < 256, text
        if gs1 and v == 0x1D:
            out.append(FNC1)
        elif v < 128:
            out.append(v + 1)
        else:
            out += [UPPER_SHIFT, v - 128 + 1]
        k += 1
    return out


def padded(cws, n):
    """the data codewords of a symbol of size n: the first pad is 129, a later one at the 1-based position p is
    129 + (149 p mod 253) + 1, less 254 where that exceeds 254"""
    cap = CAPACITY[n][0]
    assert len(cws) <= cap, (len(cws), cap)
    out = list(cws)
    while len(out) < cap:
        p = len(out) + 1
        v = PAD if len(out) == len(cws) else PAD + (149 * p) % 253 + 1
        out.append(v - 254 if v > 254 else v)
    return out


# --- placement ------------------------------------------------------------------------
@functools.lru_cache(None)
def placement(m):
    """the module map of an m x m mapping matrix (ISO/IEC 16022 Annex F): an int array, 10 * codeword (1-based) + bit (1 = the most
    significant .. 8) per module; 1 for the two dark and 0 for the two light modules of the fixed lower-right corner"""
    arr = np.zeros((m, m), np.int64)

    def module(r, c, ch, bit):
        if r < 0:
            r, c = r + m, c + 4 - (m + 4) % 8
        if c < 0:
            r, c = r + 4 - (m + 4) % 8, c + m
        assert arr[r, c] == 0
        arr[r, c] = 10 * ch + bit

    def utah(r, c, ch):
        for bit, (dr, dc) in enumerate(((-2, -2), (-2, -1), (-1, -2), (-1, -1), (-1, 0), (0, -2), (0, -1), (0, 0)), 1):
            module(r + dr, c + dc, ch, bit)

    corners = {1: ((m - 1, 0), (m - 1, 1), (m - 1, 2), (0, m - 2), (0, m - 1), (1, m - 1), (2, m - 1), (3, m - 1)),
               2: ((m - 3, 0), (m - 2, 0), (m - 1, 0), (0, m - 4), (0, m - 3), (0, m - 2), (0, m - 1), (1, m - 1)),
               3: ((m - 3, 0), (m - 2, 0), (m - 1, 0), (0, m - 2), (0, m - 1), (1, m - 1), (2, m - 1), (3, m - 1)),
               4: ((m - 1, 0), (m - 1, m - 1), (0, m - 3), (0, m - 2), (0, m - 1), (1, m - 3), (1, m - 2), (1, m - 1))}

    def corner(which, ch):
        for bit, (r, c) in enumerate(corners[which], 1):
            module(r, c, ch, bit)

    ch, r, c = 1, 4, 0
    while True:
        if r == m and c == 0:
            corner(1, ch)
            ch += 1
        if r == m - 2 and c == 0 and m % 4:
            corner(2, ch)
            ch += 1
        if r == m - 2 and c == 0 and m % 8 == 4:
            corner(3, ch)
            ch += 1
        if r == m + 4 and c == 2 and m % 8 == 0:
            corner(4, ch)
            ch += 1
        while True:                                     # up and to the right
            if r < m and c >= 0 and arr[r, c] == 0:
                utah(r, c, ch)
                ch += 1
            r, c = r - 2, c + 2
            if not (r >= 0 and c < m):
                break
        r, c = r + 1, c + 3
        while True:                                     # down and to the left
            if r >= 0 and c < m and arr[r, c] == 0:
                utah(r, c, ch)
                ch += 1
            r, c = r + 2, c - 2
            if not (r < m and c >= 0):
                break
        r, c = r + 3, c + 1
        if not (r < m or c < m):
            break
    if arr[m - 1, m - 1] == 0:
        arr[m - 1, m - 1] = arr[m - 2, m - 2] = 1
    arr.setflags(write=False)
    return arr


def symbol_from_codewords(all_cws, n):
    """(n, n) uint8, 1 = dark: finder, clock track and the placed codewords (data + check)"""
    pm = placement(n - 2)
    cw = np.asarray([0] + list(all_cws), np.int64)
    bits = np.where(pm >= 10, (cw[np.minimum(pm // 10, len(cw) - 1)] >> (8 - pm % 10)) & 1, pm)
    sym = np.zeros((n, n), np.uint8)
    sym[1:-1, 1:-1] = bits
    sym[:, 0] = 1
    sym[n - 1, :] = 1
    sym[0, 0::2] = 1
    sym[1::2, n - 1] = 1
    return sym


def symbol(text, n, gs1=False):
    data = padded(codewords(text, gs1), n)
    return symbol_from_codewords(data + check_codewords(data, CAPACITY[n][1]), n)


# --- renderer -------------------------------------------------------------------------
def _cubic(t):
    """Keys' cubic convolution kernel, a = -1/2"""
    t = np.abs(t)
    return np.where(t <= 1, (1.5 * t - 2.5) * t * t + 1, np.where(t < 2, ((-0.5 * t + 2.5) * t - 4) * t + 2, 0.0))


def _rotate_bicubic(img, angle):
    """``img`` rotated about its centre by ``angle`` degrees (clockwise on the screen), bicubic, the edge repeated"""
    h, w = img.shape
    t = np.deg2rad(angle)
    ct, st = np.cos(t), np.sin(t)
    xx = (np.arange(w) + 0.5 - w / 2.0)[None, :]
    yy = (np.arange(h) + 0.5 - h / 2.0)[:, None]
    sx, sy = ct * xx + st * yy + w / 2.0 - 0.5, -st * xx + ct * yy + h / 2.0 - 0.5
    fx, fy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    out = np.zeros((h, w))
    for j in range(-1, 3):
        wy = _cubic(sy - (fy + j))
        yi = np.clip(fy + j, 0, h - 1)
        for i in range(-1, 3):
            out += wy * _cubic(sx - (fx + i)) * img[yi, np.clip(fx + i, 0, w - 1)]
    return out


@functools.lru_cache(None)
def _drawn(sym_bytes, n, ppm, h, w, angle):
    """the float image (h, w) of the symbol upright at ``angle`` degrees, before quarter turns and degrading"""
    sym = np.frombuffer(sym_bytes, np.uint8).reshape(n, n)
    ss = 4
    canvas = np.full((h * ss, w * ss), LIGHT)
    side = n * ppm * ss
    y0, x0 = (h * ss - side) // 2, (w * ss - side) // 2
    assert y0 >= 0 and x0 >= 0, (n, ppm, h, w)
    canvas[y0:y0 + side, x0:x0 + side] = np.where(np.kron(sym, np.ones((ppm * ss, ppm * ss), np.uint8)), DARK, LIGHT)
    if angle:
        canvas = _rotate_bicubic(canvas, angle)
    return canvas.reshape(h, ss, w, ss).mean(axis=(1, 3))


def render(sym, ppm, h=128, w=128, angle=0, turns=0, blur=0.0, ramp=0.0, noise=0.0, seed=0, channels=1):
    """(h, w, channels) uint8: the (n, n) symbol at ``ppm`` whole pixels a module about the patch's centre, rotated by ``angle``
    degrees, then turned by ``turns`` quarter turns counter-clockwise (np.rot90; h == w unless turns is even), then Gaussian blur
    (sigma in pixels), an illumination ramp across x (1 -+ ramp / 2) and noise (sigma in grey levels)"""
    sym = np.ascontiguousarray(sym, np.uint8)
    img = np.rot90(_drawn(sym.tobytes(), sym.shape[0], int(ppm), h, w, angle), turns)
    if blur:
        img = _blur(img, blur)
    if ramp:
        img = img * (1.0 + ramp * (np.arange(img.shape[1]) / (img.shape[1] - 1) - 0.5))[None, :]
    if noise:
        img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape)
    grey = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(_tint(grey, channels, seed=seed))
