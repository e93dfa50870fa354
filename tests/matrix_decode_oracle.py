"""The rules of ubd_decode_matrix_patches (include/ubd.h) restated in numpy and plain integers, from the header and not from the
kernel: Data Matrix ECC 200, the square sizes 10 x 10 to 26 x 26.  tests/test_matrix_decode_host.py pins it on rendered symbols
(tests/matrix_decode_cases.py), tests/test_gpu_matrix_decode.py holds the device to it with np.array_equal."""
import functools

import numpy as np

DATAMATRIX = 32768
DEFAULTS = dict(symbologies=DATAMATRIX, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
ROW = 128
NONE = (0,) * 8 + (255,) * 120
SIZES = (10, 12, 14, 16, 18, 20, 22, 24, 26)
DATA_CHECK = {10: (3, 5), 12: (5, 7), 14: (8, 10), 16: (12, 12), 18: (18, 14), 20: (22, 18), 22: (30, 20), 24: (36, 24), 26: (44, 28)}
MIN_SIDE = 20


def luma(patch):
    p = np.asarray(patch).astype(np.int64)
    if p.shape[2] == 1:
        return p[:, :, 0]
    return (19595 * p[:, :, 0] + 38470 * p[:, :, 1] + 7471 * p[:, :, 2] + 0x8000) >> 16


def dark_map(patch, band, window, contrast):
    """rule 1 -> (H, W) bool"""
    g = luma(patch)
    h, w = g.shape
    m = (2 * band + 1) ** 2
    ys, xs = np.arange(h), np.arange(w)
    s = np.zeros_like(g)
    for dy in range(-band, band + 1):
        for dx in range(-band, band + 1):
            s += g[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)]
    lo, hi = s.copy(), s.copy()
    for axis, size in ((1, w), (0, h)):
        src_lo, src_hi = lo.copy(), hi.copy()
        for k in range(1, window + 1):                  # clipping the square: an index beyond the patch repeats one inside it
            for idx in (np.clip(np.arange(size) + k, 0, size - 1), np.clip(np.arange(size) - k, 0, size - 1)):
                lo = np.minimum(lo, np.take(src_lo, idx, axis=axis))
                hi = np.maximum(hi, np.take(src_hi, idx, axis=axis))
    d = 2 * m * g - lo - hi
    d = np.where(hi - lo < contrast * m, np.maximum(d, 1), d)
    return d < -contrast * m


def _extent(counts):
    """rule 2 on one axis -> (first, last) or None"""
    t = max(1, int(counts.max()) // 4)
    at = np.nonzero(counts >= t)[0]
    return (int(at[0]), int(at[-1])) if len(at) else None


def _anchors(values, a0, a1, largest):
    """rule 3 for one side: values[a] for a in a0..a1 (-1: skipped) -> ((c1, p1), (c2, p2)) in 1/16 pixel, or None"""
    n = a1 - a0 + 1
    out = []
    for s0, s1 in ((a0 + n // 16, a0 + n // 2 - 1), (a1 - n // 2 + 1, a1 - n // 16)):
        v = [int(values[a]) for a in range(s0, s1 + 1) if values[a] >= 0]
        if len(v) < 4:
            return None
        v.sort(reverse=largest)
        out.append((8 * (s0 + s1 + 1), 16 * v[len(v) // 4]))
    return tuple(out)


def _line(anchors, c):
    (c1, p1), (c2, p2) = anchors
    return min(max(p1 + ((p2 - p1) * (c - c1)) // (c2 - c1), -32768), 32767)        # Python's // floors; the clamp keeps int32 exact


def locate(dark):
    """rules 2..4 -> the corners ((xTL, yTL), (xTR, yTR), (xBL, yBL), (xBR, yBR)) in 1/16 pixel, or None"""
    ex, ey = _extent(dark.sum(axis=0)), _extent(dark.sum(axis=1))
    if ex is None or ey is None:
        return None
    (x0, x1), (y0, y1) = ex, ey
    if x1 - x0 + 1 < MIN_SIDE or y1 - y0 + 1 < MIN_SIDE:
        return None
    h, w = dark.shape
    box = dark[y0:y1 + 1, x0:x1 + 1]
    left, right, top, bottom = np.full(h, -1), np.full(h, -1), np.full(w, -1), np.full(w, -1)
    for y in range(y0, y1 + 1):
        at = np.nonzero(box[y - y0])[0]
        if len(at):
            left[y], right[y] = x0 + at[0], x0 + at[-1] + 1
    for x in range(x0, x1 + 1):
        at = np.nonzero(box[:, x - x0])[0]
        if len(at):
            top[x], bottom[x] = y0 + at[0], y0 + at[-1] + 1
    sides = (_anchors(left, y0, y1, False), _anchors(right, y0, y1, True), _anchors(top, x0, x1, False), _anchors(bottom, x0, x1, True))
    if any(s is None for s in sides):
        return None
    a_left, a_right, a_top, a_bottom = sides
    corners = []
    for horizontal, vertical in ((a_top, a_left), (a_top, a_right), (a_bottom, a_left), (a_bottom, a_right)):
        y = _line(horizontal, 8 * (x0 + x1 + 1))
        for _ in range(3):
            x = _line(vertical, y)
            y = _line(horizontal, x)
        corners.append((x, y))
    return tuple(corners)


def sample(dark, corners, n, r, c):
    """rule 5: module (r, c) of an n x n grid"""
    (xa, ya), (xb, yb), (xc, yc), (xd, yd) = corners
    big, u, v = 2 * n, 2 * c + 1, 2 * r + 1
    x = ((big - u) * (big - v) * xa + u * (big - v) * xb + (big - u) * v * xc + u * v * xd) // (big * big)
    y = ((big - u) * (big - v) * ya + u * (big - v) * yb + (big - u) * v * yc + u * v * yd) // (big * big)
    h, w = dark.shape
    return bool(dark[min(max(y >> 4, 0), h - 1), min(max(x >> 4, 0), w - 1)])


def canonical(n, turns, r, c):
    """where module (r, c) of the sampled grid lies in the symbol, if the patch shows the symbol turned by ``turns`` quarter
    turns counter-clockwise"""
    return ((r, c), (c, n - 1 - r), (n - 1 - r, n - 1 - c), (n - 1 - c, r))[turns]


def border_dark(n, r, c):
    """the canonical border: the left column and the bottom row dark, the top row dark at even columns, the right column at odd rows"""
    if c == 0 or r == n - 1:
        return True
    return c % 2 == 0 if r == 0 else r % 2 == 1


def finder(dark, corners):
    """rule 6 -> (n, turns, mismatches) or None"""
    miss = []
    for n in SIZES:
        border = [(r, c) for r in range(n) for c in range(n) if r in (0, n - 1) or c in (0, n - 1)]
        got = [sample(dark, corners, n, r, c) for r, c in border]
        for t in range(4):
            miss.append((sum(g != border_dark(n, *canonical(n, t, r, c)) for g, (r, c) in zip(got, border)), n, t))
    best = min(miss)
    if 8 * best[0] > 4 * best[1] - 4 or sum(1 for m in miss if m[0] == best[0]) != 1:
        return None
    return best[1], best[2], best[0]


def read_codewords(grid):
    """rule 7: the (n, n) canonical grid (bool) -> the data + check codewords, by walking ISO/IEC 16022 Annex F's placement"""
    n = grid.shape[0]
    m = n - 2
    seen = np.zeros((m, m), bool)
    out = []

    def bit(r, c):
        if r < 0:
            r += m
            c += 4 - (m + 4) % 8
        if c < 0:
            c += m
            r += 4 - (m + 4) % 8
        seen[r, c] = True
        return int(grid[r + 1, c + 1])

    def word(cells):
        v = 0
        for r, c in cells:
            v = 2 * v + bit(r, c)
        out.append(v)

    def utah(r, c):
        word(((r - 2, c - 2), (r - 2, c - 1), (r - 1, c - 2), (r - 1, c - 1), (r - 1, c), (r, c - 2), (r, c - 1), (r, c)))

    r, c = 4, 0
    while True:
        if r == m and c == 0:
            word(((m - 1, 0), (m - 1, 1), (m - 1, 2), (0, m - 2), (0, m - 1), (1, m - 1), (2, m - 1), (3, m - 1)))
        if r == m - 2 and c == 0 and m % 4 != 0:
            word(((m - 3, 0), (m - 2, 0), (m - 1, 0), (0, m - 4), (0, m - 3), (0, m - 2), (0, m - 1), (1, m - 1)))
        if r == m - 2 and c == 0 and m % 8 == 4:
            word(((m - 3, 0), (m - 2, 0), (m - 1, 0), (0, m - 2), (0, m - 1), (1, m - 1), (2, m - 1), (3, m - 1)))
        if r == m + 4 and c == 2 and m % 8 == 0:
            word(((m - 1, 0), (m - 1, m - 1), (0, m - 3), (0, m - 2), (0, m - 1), (1, m - 3), (1, m - 2), (1, m - 1)))
        while True:
            if r < m and c >= 0 and not seen[r, c]:
                utah(r, c)
            r, c = r - 2, c + 2
            if r < 0 or c >= m:
                break
        r, c = r + 1, c + 3
        while True:
            if r >= 0 and c < m and not seen[r, c]:
                utah(r, c)
            r, c = r + 2, c - 2
            if r >= m or c < 0:
                break
        r, c = r + 3, c + 1
        if r >= m and c >= m:
            break
    assert len(out) == sum(DATA_CHECK[n])
    return out


# --- GF(256) with the polynomial 0x12D ---------------------------------------------------
@functools.lru_cache(None)
def _tables():
    exp, log, v = [0] * 510, [0] * 256, 1
    for k in range(255):
        exp[k] = exp[k + 255] = v
        log[v] = k
        v <<= 1
        if v & 0x100:
            v ^= 0x12D
    return exp, log


def _mul(a, b):
    exp, log = _tables()
    return exp[log[a] + log[b]] if a and b else 0


def _inv(a):
    exp, log = _tables()
    return exp[255 - log[a]]


def _poly_at(coeffs_low_first, x):
    v = 0
    for cf in reversed(coeffs_low_first):
        v = _mul(v, x) ^ cf
    return v


def syndromes(word, e):
    exp, _ = _tables()
    return [_poly_at(list(reversed(word)), exp[j]) for j in range(1, e + 1)]


def reed_solomon(word, e):
    """rule 8: the received codewords (data then check, the first the highest power) -> (corrected word, number corrected) or None"""
    exp, _ = _tables()
    n = len(word)
    syn = syndromes(word, e)
    if not any(syn):
        return list(word), 0
    lam, prev, big_l, shift, b = [1], [1], 0, 1, 1       # Berlekamp-Massey
    for k in range(e):
        delta = syn[k]
        for i in range(1, big_l + 1):
            if i < len(lam):
                delta ^= _mul(lam[i], syn[k - i])
        if delta == 0:
            shift += 1
            continue
        scale = _mul(delta, _inv(b))
        new = list(lam) + [0] * max(0, len(prev) + shift - len(lam))
        for i, cf in enumerate(prev):
            new[i + shift] ^= _mul(scale, cf)
        if 2 * big_l <= k:
            prev, big_l, b, shift = lam, k + 1 - big_l, delta, 1
        else:
            shift += 1
        lam = new
    while len(lam) > 1 and lam[-1] == 0:
        lam.pop()
    degree = len(lam) - 1
    if big_l > e // 2 or degree != big_l:
        return None
    roots = [p for p in range(n) if _poly_at(lam, exp[(255 - p) % 255]) == 0]     # p: the power of x the codeword stands at
    if len(roots) != degree:
        return None
    omega = [0] * e
    for i in range(e):
        for j in range(min(i, degree) + 1):
            omega[i] ^= _mul(lam[j], syn[i - j])
    fixed = list(word)
    for p in roots:
        xinv = exp[(255 - p) % 255]
        deriv = 0
        for i in range(1, degree + 1, 2):               # the formal derivative keeps the odd terms
            deriv ^= _mul(lam[i], _pow(xinv, i - 1))
        if deriv == 0:
            return None
        fixed[n - 1 - p] ^= _mul(_poly_at(omega, xinv), _inv(deriv))
    if any(syndromes(fixed, e)):
        return None
    return fixed, degree


def _pow(a, k):
    exp, log = _tables()
    return 1 if k == 0 else (exp[(log[a] * k) % 255] if a else 0)


def read_text(data):
    """rule 9: the data codewords -> (elements, flags, raw)"""
    elements, flags, k = [], 0, 0
    while k < len(data):
        cw = data[k]
        if 1 <= cw <= 128:
            elements.append(cw - 1)
        elif 130 <= cw <= 229:
            elements += [48 + (cw - 130) // 10, 48 + (cw - 130) % 10]
        elif cw == 235 and k + 1 < len(data) and 1 <= data[k + 1] <= 128:
            elements.append(data[k + 1] + 127)
            k += 1
        elif cw == 129:
            return elements, flags, []
        elif cw == 232 and k == 0:
            flags |= 1
        elif cw == 232:
            elements.append(0x1D)
        else:
            return elements, flags | 2, list(data[k:])
        k += 1
    return elements, flags, []


def make_row(n, turns, corrected, mismatches, data):
    elements, flags, raw = read_text(data)
    row = [68, n, turns, len(elements), flags, corrected, mismatches, len(raw)] + elements + raw
    return row + [255] * (ROW - len(row))


def decode_bitmap(dark):
    """rules 2..9 on a dark map -> the 128 bytes of the row, as a list"""
    corners = locate(dark)
    if corners is None:
        return list(NONE)
    found = finder(dark, corners)
    if found is None:
        return list(NONE)
    n, turns, mismatches = found
    grid = np.zeros((n, n), bool)
    for r in range(n):
        for c in range(n):
            grid[canonical(n, turns, r, c)] = sample(dark, corners, n, r, c)
    data_n, e = DATA_CHECK[n]
    fixed = reed_solomon(read_codewords(grid), e)
    if fixed is None:
        return list(NONE)
    return make_row(n, turns, fixed[1], mismatches, fixed[0][:data_n])


def decode_patch(patch, **kw):
    p = dict(DEFAULTS, **kw)
    assert p["symbologies"] == DATAMATRIX
    return decode_bitmap(dark_map(patch, p["band"], p["window"], p["contrast"]))


def decode_patches(patches, counts, fill, **kw):
    """(n, cap, h, w, c) uint8 and counts -> (n, cap, 128) uint8; rows of slots that hold no object keep ``fill``"""
    n, cap = patches.shape[:2]
    out = np.full((n, cap, ROW), fill, np.uint8)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            out[i, j] = decode_patch(patches[i, j], **kw)
    return out
