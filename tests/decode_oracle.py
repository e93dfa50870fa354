"""Numpy restatement of ubd_decode_patches (include/ubd.h), written from its specification and not from the kernel: luma, scan
lines, local threshold, sub-pixel edges, candidates, edge-to-similar-edge characters, checksums and votes of the retail family
(EAN-13 with UPC-A, EAN-8).  Everything is integer arithmetic on Python integers (exact); divisions floor, and every dividend
is non-negative.  tests/test_decode_host.py pins it on rendered symbols; the device is compared with ``decode_patches`` by
tests/test_gpu_decode.py with np.array_equal."""
import numpy as np

EAN13, EAN8 = 1, 2                                        # bits of ``symbologies``
DEFAULTS = dict(symbologies=EAN13 | EAN8, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)

# run widths in scan order for the digits 0..9: set L (a space first), set R the same widths (a bar first), set G = L reversed
L_WIDTHS = [tuple(int(ch) for ch in s) for s in "3211 2221 2122 1411 1132 1231 1114 1312 1213 3112".split()]
G_WIDTHS = [w[::-1] for w in L_WIDTHS]
PARITY_WORDS = "LLLLLL LLGLGG LLGGLG LLGGGL LGLLGG LGGLLG LGGGLL LGLGLG LGLGGL LGGLGL".split()
# symbology bit -> (result code, runs, modules, characters per half)
LAYOUT = {EAN13: (13, 59, 95, 6), EAN8: (8, 43, 67, 4)}


def luma(patch):
    """(h, w) or (h, w, 1) or (h, w, 3) uint8 -> (h, w) Python-exact int64 luma, Pillow's convert('L')"""
    a = np.asarray(patch).astype(np.int64)
    if a.ndim == 2:
        return a
    if a.shape[2] == 1:
        return a[:, :, 0]
    return (19595 * a[:, :, 0] + 38470 * a[:, :, 1] + 7471 * a[:, :, 2] + 0x8000) >> 16


def line_profile(lum, k, scan_rows, band):
    """scan line k -> (p, m): the luma sums over the rows [r_k - band, r_k + band] clipped to the patch, and the row count"""
    h = lum.shape[0]
    r = ((2 * k + 1) * h) // (2 * scan_rows)
    r0, r1 = max(0, r - band), min(h - 1, r + band)
    return [int(v) for v in lum[r0:r1 + 1].sum(axis=0)], r1 - r0 + 1


def line_d(p, m, window, contrast):
    w = len(p)
    d = []
    for x in range(w):
        seg = p[max(0, x - window):min(w - 1, x + window) + 1]
        lo, hi = min(seg), max(seg)
        v = 2 * p[x] - lo - hi
        if hi - lo < contrast * m:
            v = max(v, 1)
        d.append(v)
    return d


def line_edges(d):
    """-> (e, l2d): positions in 1/256 pixel and whether each edge goes from light to dark"""
    e, l2d = [], []
    for x in range(len(d) - 1):
        if (d[x] < 0) != (d[x + 1] < 0):
            a, b = abs(d[x]), abs(d[x + 1])
            e.append(256 * x + (256 * a) // (a + b))
            l2d.append(d[x + 1] < 0)
    return e, l2d


def mirror(e, l2d, w):
    """reverse reading: the mirrored edge list, polarities swapped"""
    n = len(e)
    return [256 * (w - 1) - e[n - 1 - j] for j in range(n)], [not l2d[n - 1 - j] for j in range(n)]


def decode_character(w4, sets):
    """four run widths, allowed sets (a string of 'L', 'G'; 'R' reads as 'L') -> (set, digit) or None"""
    s4 = sum(w4)
    if s4 <= 0:
        return None
    e1 = (14 * (w4[0] + w4[1]) + s4) // (2 * s4)
    e2 = (14 * (w4[1] + w4[2]) + s4) // (2 * s4)
    if not (2 <= e1 <= 5 and 2 <= e2 <= 5):
        return None
    best, best_cost, ties = None, None, 0
    for name in sets:
        table = G_WIDTHS if name == "G" else L_WIDTHS
        for digit, n in enumerate(table):
            if n[0] + n[1] == e1 and n[1] + n[2] == e2:
                cost = abs(7 * (w4[0] + w4[2]) - s4 * (n[0] + n[2]))
                if best_cost is None or cost < best_cost:
                    best, best_cost, ties = (name, digit), cost, 1
                elif cost == best_cost:
                    ties += 1
    return best if ties == 1 else None


def decode_candidate(e, l2d, i, sym, quiet):
    """candidate start edge i of symbology bit ``sym`` -> the digits (list) or None"""
    code, runs, modules, half = LAYOUT[sym]
    n = len(e)
    if not l2d[i] or i + runs >= n:
        return None
    st = e[i + runs] - e[i]
    if st <= 0:
        return None
    if i >= 1 and modules * (e[i] - e[i - 1]) < quiet * st:
        return None
    if i + runs + 1 < n and modules * (e[i + runs + 1] - e[i + runs]) < quiet * st:
        return None
    w = [e[i + j + 1] - e[i + j] for j in range(runs)]
    centre = 3 + 4 * half
    for j in list(range(3)) + list(range(centre, centre + 5)) + list(range(runs - 3, runs)):
        if (2 * modules * w[j] + st) // (2 * st) != 1:
            return None
    left = [decode_character(w[3 + 4 * k:7 + 4 * k], "LG" if sym == EAN13 else "L") for k in range(half)]
    right = [decode_character(w[centre + 5 + 4 * k:centre + 9 + 4 * k], "R") for k in range(half)]
    if None in left or None in right:
        return None
    digits = [c[1] for c in left] + [c[1] for c in right]
    if sym == EAN13:
        word = "".join(c[0] for c in left)
        if word not in PARITY_WORDS:
            return None
        digits = [PARITY_WORDS.index(word)] + digits
        check = (10 - (sum(digits[0:12:2]) + 3 * sum(digits[1:12:2])) % 10) % 10
    else:
        check = (10 - (3 * sum(digits[0:7:2]) + sum(digits[1:7:2])) % 10) % 10
    return digits if check == digits[-1] else None


def line_votes(e, l2d, w, symbologies, quiet):
    """one scan line -> [(direction bit, result code, digits tuple)]: per (direction, symbology) the valid candidate with the lowest start"""
    votes = []
    for bit, (ee, pp) in ((1, (e, l2d)), (2, mirror(e, l2d, w))):
        for sym in (EAN13, EAN8):
            if symbologies & sym:
                for i in range(len(ee)):
                    digits = decode_candidate(ee, pp, i, sym, quiet)
                    if digits is not None:
                        votes.append((bit, LAYOUT[sym][0], tuple(digits)))
                        break
    return votes


def tally(votes, min_votes):
    """all votes of a patch -> the result row of 16 integers"""
    none = [0, 0, 0] + [-1] * 13
    count, mask = {}, {}
    for bit, code, digits in votes:
        key = (code, digits)
        count[key] = count.get(key, 0) + 1
        mask[key] = mask.get(key, 0) | bit
    if not count:
        return none
    top = max(count.values())
    winners = [k for k, v in count.items() if v == top]
    if top < min_votes or len(winners) != 1:
        return none
    code, digits = winners[0]
    return [code, top, mask[winners[0]]] + list(digits) + [-1] * (13 - len(digits))


def decode_patch(patch, symbologies=3, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2):
    lum = luma(patch)
    w = lum.shape[1]
    votes = []
    for k in range(scan_rows):
        p, m = line_profile(lum, k, scan_rows, band)
        e, l2d = line_edges(line_d(p, m, window, contrast))
        votes += line_votes(e, l2d, w, symbologies, quiet)
    return tally(votes, min_votes)


def decode_patches(patches, counts, fill, **params):
    """(n, cap, h, w, c) uint8, counts (n) -> int32 (n, cap, 16); rows of slots j >= min(counts[i], cap) keep ``fill``"""
    patches = np.asarray(patches)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, 16), fill, np.int32)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            out[i, j] = decode_patch(patches[i, j], **params)
    return out
