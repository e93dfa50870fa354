"""Test symbols for the decoder: an encoder of the retail family from the public 7-module tables (EAN-13 / UPC-A / EAN-8;
independent of the run-width tables of tests/decode_oracle.py) and a renderer that draws a symbol into a frame at any angle,
super-sampled, with optional blur, noise and an illumination ramp, and returns the true corners of the bar area."""
import numpy as np

# the left-hand odd-parity characters (set A / L) as seven modules, 1 = dark; R is the complement, G is R mirrored
L_CODES = ["0001101", "0011001", "0010011", "0111101", "0100011", "0110001", "0101111", "0111011", "0110111", "0001011"]
R_CODES = ["".join("1" if ch == "0" else "0" for ch in s) for s in L_CODES]
G_CODES = [s[::-1] for s in R_CODES]
PARITY = ["LLLLLL", "LLGLGG", "LLGGLG", "LLGGGL", "LGLLGG", "LGGLLG", "LGGGLL", "LGLGLG", "LGLGGL", "LGGLGL"]
CLEAN = dict(blur=0.0, noise=0.0, ramp=0.0)
HARD = dict(blur=0.6, noise=4.0, ramp=0.25)


def check_digit(body):
    """the check digit of 12 (EAN-13) or 7 (EAN-8) digits: weights 3 and 1 alternate, the digit next to the check weighs 3"""
    total = sum(d * (3 if k % 2 == 0 else 1) for k, d in enumerate(reversed(body)))
    return (10 - total % 10) % 10


def with_check(body):
    body = [int(d) for d in body]
    assert len(body) in (12, 7)
    return body + [check_digit(body)]


def modules(digits):
    """13 or 8 digits -> the 95 or 67 modules of the symbol as a string of 0 / 1 (no quiet zone)"""
    digits = [int(d) for d in digits]
    if len(digits) == 13:
        left = "".join((L_CODES if p == "L" else G_CODES)[d] for p, d in zip(PARITY[digits[0]], digits[1:7]))
        right = "".join(R_CODES[d] for d in digits[7:])
    else:
        assert len(digits) == 8
        left = "".join(L_CODES[d] for d in digits[:4])
        right = "".join(R_CODES[d] for d in digits[4:])
    return "101" + left + "01010" + right + "101"


def runs(digits):
    """13 or 8 digits -> the run widths in modules, the first run being the first bar of the start guard"""
    m = modules(digits)
    out, n = [], 1
    for a, b in zip(m, m[1:]):
        if a == b:
            n += 1
        else:
            out.append(n)
            n = 1
    return out + [n]


def edges_from_runs(widths, unit=256 * 3, start=256 * 20, grow=0):
    """run widths in modules -> edge positions in 1/256 pixel; ``grow`` widens every bar by that much (ink spread) and narrows
    the spaces alike; the first edge goes from light to dark"""
    e, pos = [start - grow // 2], start
    for k, w in enumerate(widths):
        pos += w * unit
        e.append(pos + (grow // 2 if k % 2 == 0 else -(grow // 2)))
    return e


def flat_row(symbols, px_per_module, width, start, gap=0, light=225, dark=35):
    """one uint8 row of ``width`` pixels: the symbols (digit lists) drawn upright side by side at whole pixels per module, the
    first at column ``start``, ``gap`` light pixels between two"""
    row = np.full(width, light, np.uint8)
    x = start
    for digits in symbols:
        for ch in modules(digits):
            if ch == "1":
                row[x:x + px_per_module] = dark
            x += px_per_module
        x += gap
    assert x - gap <= width
    return row


def flat_patch(symbols, px_per_module, height, width, start, gap=0, channels=1):
    """(height, width, channels) uint8: ``flat_row`` on every row"""
    row = flat_row(symbols, px_per_module, width, start, gap)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (height, width, channels)))


# The four helpers below are those of the GPU tests of both decoder families (tests/test_gpu_decode.py, tests/test_gpu_text_decode.py),
# which import them under these names.
def _tint(grey, c, seed=0):
    """(.., h, w) uint8 -> (.., h, w, c): for c = 3 three different channel gains, so that the luma weights matter"""
    if c == 1:
        return grey[..., None]
    gains = np.random.default_rng(seed).uniform(0.6, 1.0, 3)
    return (grey[..., None].astype(np.float64) * gains).astype(np.uint8)


def _stripes(rng, h, w, lo=1, hi=8):
    row, x, v = np.zeros(w, np.uint8), 0, 0
    while x < w:
        k = int(rng.integers(lo, hi + 1))
        row[x:x + k] = 225 if v else 35
        x, v = x + k, 1 - v
    return np.broadcast_to(row[None, :], (h, w)).copy()


def _noisy(rng, grey, sigma=6.0):
    return np.clip(np.rint(grey + rng.normal(0, sigma, grey.shape)), 0, 255).astype(np.uint8)


def _row_from_pixel_runs(runs_px, width, start):
    row, x = np.full(width, 225, np.uint8), start
    for k, w in enumerate(runs_px):
        if k % 2 == 0:
            row[x:x + w] = 35
        x += w
    assert x <= width
    return row


def _blur(img, sigma):
    r = 3
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        pad = [(r, r) if a == axis else (0, 0) for a in (0, 1)]
        p = np.pad(img, pad, mode="edge")
        img = sum(k[t] * np.take(p, np.arange(t, t + img.shape[axis]), axis=axis) for t in range(2 * r + 1))
    return img


def render(digits, px_per_module, angle=0.0, aspect=0.3, margin_modules=14, supersample=4, blur=0.0, noise=0.0, ramp=0.0,
           seed=0, light=225.0, dark=35.0):
    """-> (frame (h, w) uint8, quad): the symbol drawn about the frame's centre, rotated by ``angle`` degrees (clockwise on the
    screen); quad = the four corners of the BAR area (no quiet zone) as 8 floats, clockwise from the corner where the symbol's
    first bar begins, in the continuous coordinates in which pixel (x, y) covers [x, x + 1) x [y, y + 1)."""
    m = np.array([int(ch) for ch in modules(digits)], np.int64)
    width, height = len(m) * float(px_per_module), len(m) * float(px_per_module) * aspect
    side = int(np.ceil(np.hypot(width + 2 * margin_modules * px_per_module, height + 2 * margin_modules * px_per_module))) + 8
    side += -side % 4
    c = side / 2.0
    t = np.deg2rad(angle)
    ct, st = np.cos(t), np.sin(t)
    sub = (np.arange(side * supersample) + 0.5) / supersample
    xx, yy = sub[None, :] - c, sub[:, None] - c
    u, v = ct * xx + st * yy + width / 2, -st * xx + ct * yy
    idx = np.clip(np.floor(u / px_per_module).astype(np.int64), 0, len(m) - 1)
    bar = (u >= 0) & (u < width) & (np.abs(v) <= height / 2) & (m[idx] == 1)
    img = np.where(bar, dark, light).reshape(side, supersample, side, supersample).mean(axis=(1, 3))
    if blur:
        img = _blur(img, blur)
    if ramp:
        img = img * (1.0 + ramp * (2.0 * np.arange(side) / (side - 1) - 1.0))[None, :]
    if noise:
        img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape)
    frame = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    quad = []
    for uu, vv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        a, b = uu * width / 2, vv * height / 2
        quad += [c + ct * a - st * b, c + st * a + ct * b]
    return frame, quad


def int_quad(quad):
    return [int(round(v)) for v in quad]
