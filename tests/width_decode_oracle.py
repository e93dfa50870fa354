"""Numpy restatement of ubd_decode_width_patches (include/ubd.h), written from its specification and not from the kernel: the
two-width family, Interleaved 2 of 5 (ITF) and Code 39.  Every run of a group is narrow or wide against the group's own least and
greatest run; ITF pairs of five bars and five spaces, Code 39 characters of nine runs, the candidates, the optional checks, the
votes over (symbology, all elements) and the row of the winner.  Luma, scan lines, local threshold, sub-pixel edges and the
mirrored list are those of ubd_decode_patches and come from tests/decode_oracle.py.  Everything is integer arithmetic on Python
integers (exact), and no rule divides.  tests/test_width_decode_host.py pins it on rendered symbols; the device is compared with
``decode_patches`` by tests/test_gpu_width_decode.py with np.array_equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_oracle import luma, line_profile, line_d, line_edges, mirror  # noqa: E402

ITF, CODE39 = 8, 16                                       # bits 3 and 4 of ``symbologies``
DEFAULTS = dict(symbologies=ITF | CODE39, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
ROW = 128                                                 # bytes of a result row
CODE_ITF, CODE_39 = 25, 39                                # byte 0 of a result row
MAX_PAIRS, MIN_PAIRS, MAX_CHARS = 30, 3, 60

# ITF: the five runs of one colour for the digits 0..9
ITF_PATTERNS = "nnWWn WnnnW nWnnW WWnnn nnWnW WnWnn nWWnn nnnWW WnnWn nWnWn".split()
ITF_DIGITS = {p: d for d, p in enumerate(ITF_PATTERNS)}
# Code 39: bar columns 1..10, four space patterns for the forty characters that have two wide bars, four characters of wide spaces
_COLUMNS = "WnnnW nWnnW WWnnn nnWnW WnWnn nWWnn nnnWW WnnWn nWnWn nnWWn".split()
_GROUPS = [("1234567890", "nWnn"), ("ABCDEFGHIJ", "nnWn"), ("KLMNOPQRST", "nnnW"), ("UVWXYZ-. *", "Wnnn")]


def _weave(bars, spaces):
    return "".join(b + s for b, s in zip(bars, spaces + " ")).strip()


C39_PATTERNS = {}                                         # nine runs, a bar first -> the character
for _chars, _spaces in _GROUPS:
    for _ch, _bars in zip(_chars, _COLUMNS):
        C39_PATTERNS[_weave(_bars, _spaces)] = _ch
for _ch, _spaces in zip("$/+%", "WWWn WWnW WnWW nWWW".split()):
    C39_PATTERNS[_weave("nnnnn", _spaces)] = _ch
C39_VALUES = {ch: v for v, ch in enumerate("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%")}
assert len(C39_PATTERNS) == 44 and len(C39_VALUES) == 43


def classify(runs):
    """a group of runs -> (pattern string of n / W, lo, hi), or None where the wide runs are not clear of the narrow ones"""
    lo, hi = min(runs), max(runs)
    wide = [2 * w > lo + hi for w in runs]
    if not any(wide):
        return None
    if 2 * min(w for w, f in zip(runs, wide) if f) < 3 * max(w for w, f in zip(runs, wide) if not f):
        return None
    return "".join("W" if f else "n" for f in wide), lo, hi


def decode_pair(w10):
    """ten run widths, a bar first -> (first digit, second digit, (lo, hi) of the bars, (lo, hi) of the spaces) or None"""
    out = []
    for group in (w10[0::2], w10[1::2]):
        c = classify(group)
        if c is None or c[0].count("W") != 2 or c[0] not in ITF_DIGITS:
            return None
        out.append((ITF_DIGITS[c[0]], (c[1], c[2])))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def decode_character(w9):
    """nine run widths, a bar first -> (character, N6) or None"""
    c = classify(w9)
    if c is None or c[0].count("W") != 3 or c[0] not in C39_PATTERNS:
        return None
    return C39_PATTERNS[c[0]], sum(w for w, f in zip(w9, c[0]) if f == "n")


def _widths(e, j, count):
    return [e[j + k + 1] - e[j + k] for k in range(count)]


def itf_candidate(e, l2d, i, quiet):
    """candidate start edge i -> the ASCII codes of its digits, or None"""
    n = len(e)
    if not l2d[i] or i + 4 >= n:
        return None
    s4 = e[i + 4] - e[i]
    if i >= 1 and 4 * (e[i] - e[i - 1]) < quiet * s4:
        return None
    digits, j, s_prev, first, last = [], i + 4, 0, None, None
    while True:
        pair = decode_pair(_widths(e, j, 10)) if j + 10 < n else None
        if pair is not None and digits and not 7 * s_prev <= 8 * (e[j + 10] - e[j]) <= 9 * s_prev:
            pair = None
        if pair is None:
            break                                                       # j must be the stop
        if len(digits) == 2 * MAX_PAIRS:
            return None
        digits += [pair[0], pair[1]]
        last = pair[2:]
        first = first or last
        s_prev, j = e[j + 10] - e[j], j + 10
    if len(digits) < 2 * MIN_PAIRS:
        return None
    for k, w in enumerate(_widths(e, i, 4)):
        lo, hi = first[k % 2]
        if not lo <= 2 * w <= lo + hi:
            return None
    if j + 3 >= n:
        return None
    bar, space, end = _widths(e, j, 3)
    (lo_b, hi_b), (lo_s, hi_s) = last
    if not 2 * bar > lo_b + hi_b or not lo_s <= 2 * space <= lo_s + hi_s or not lo_b <= 2 * end <= lo_b + hi_b:
        return None
    if j + 4 < n and 2 * (e[j + 4] - e[j + 3]) < quiet * (space + end):
        return None
    return [48 + d for d in digits]


def c39_candidate(e, l2d, i, quiet):
    """candidate start edge i -> the ASCII codes of its data characters, or None"""
    n = len(e)
    if not l2d[i] or i + 9 >= n:
        return None
    start = decode_character(_widths(e, i, 9))
    if start is None or start[0] != "*":
        return None
    n6, s_prev = start[1], e[i + 9] - e[i]
    if i >= 1 and 6 * (e[i] - e[i - 1]) < quiet * n6:
        return None
    text, j = [], i + 10
    while True:
        if j + 9 >= n:
            return None
        g, s = e[j] - e[j - 1], e[j + 9] - e[j]
        if not (n6 <= 12 * g and 2 * g <= s_prev):
            return None
        if not 7 * s_prev <= 8 * s <= 9 * s_prev:
            return None
        ch = decode_character(_widths(e, j, 9))
        if ch is None:
            return None
        n6, s_prev = ch[1], s
        if ch[0] == "*":
            break
        if len(text) == MAX_CHARS:
            return None
        text.append(ord(ch[0]))
        j += 10
    if not text:
        return None
    if j + 10 < n and 6 * (e[j + 10] - e[j + 9]) < quiet * n6:
        return None
    return text


def check_holds(code, elements):
    """flag bit 0: the optional check character holds (GS1's modulo 10 for ITF, modulo 43 for Code 39)"""
    t = len(elements)
    if code == CODE_ITF:
        d = [v - 48 for v in elements]
        return (d[-1] + sum(v * (3 if (t - 1 - k) % 2 else 1) for k, v in enumerate(d[:-1]))) % 10 == 0
    values = [C39_VALUES[chr(v)] for v in elements]
    return t >= 2 and sum(values[:-1]) % 43 == values[-1]


def line_votes(e, l2d, w, symbologies, quiet):
    """one scan line -> [(direction bit, code, elements tuple)]: per (direction, symbology) the valid candidate with the lowest start"""
    votes = []
    for bit, (ee, pp) in ((1, (e, l2d)), (2, mirror(e, l2d, w))):
        for sym, code, candidate in ((ITF, CODE_ITF, itf_candidate), (CODE39, CODE_39, c39_candidate)):
            if symbologies & sym:
                for i in range(len(ee)):
                    elements = candidate(ee, pp, i, quiet)
                    if elements is not None:
                        votes.append((bit, code, tuple(elements)))
                        break
    return votes


def none_row():
    return [0] * 8 + [0xFF] * (ROW - 8)


def tally(votes, min_votes):
    """all votes of a patch -> the result row of 128 bytes"""
    count, mask = {}, {}
    for bit, code, elements in votes:
        key = (code, elements)
        count[key] = count.get(key, 0) + 1
        mask[key] = mask.get(key, 0) | bit
    if not count:
        return none_row()
    top = max(count.values())
    winners = [k for k, v in count.items() if v == top]
    if top < min_votes or len(winners) != 1:
        return none_row()
    code, elements = winners[0]
    head = [code, top, mask[winners[0]], len(elements), int(check_holds(code, elements)), 0, 0, 0]
    return head + list(elements) + [0xFF] * (ROW - 8 - len(elements))


def decode_patch(patch, symbologies=ITF | CODE39, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2):
    assert symbologies in (ITF, CODE39, ITF | CODE39)
    lum = luma(patch)
    w = lum.shape[1]
    votes = []
    for k in range(scan_rows):
        p, m = line_profile(lum, k, scan_rows, band)
        e, l2d = line_edges(line_d(p, m, window, contrast))
        votes += line_votes(e, l2d, w, symbologies, quiet)
    return tally(votes, min_votes)


def decode_patches(patches, counts, fill, **params):
    """(n, cap, h, w, c) uint8, counts (n) -> uint8 (n, cap, 128); rows of slots j >= min(counts[i], cap) keep ``fill``"""
    patches = np.asarray(patches)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, ROW), fill, np.uint8)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            out[i, j] = decode_patch(patches[i, j], **params)
    return out
