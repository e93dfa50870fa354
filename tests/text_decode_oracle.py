"""Numpy restatement of ubd_decode_text_patches (include/ubd.h), written from its specification and not from the kernel: the
Code 128 / GS1-128 candidates, edge-to-similar-edge characters of six runs, the modulo-103 check, the votes over whole value
sequences and the text of the winner.  Luma, scan lines, local threshold, sub-pixel edges and the mirrored list are those of
ubd_decode_patches and come from tests/decode_oracle.py.  Everything is integer arithmetic on Python integers (exact); divisions
floor, and every dividend is non-negative.  tests/test_text_decode_host.py pins it on rendered symbols; the device is compared
with ``decode_patches`` by tests/test_gpu_text_decode.py with np.array_equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_oracle import luma, line_profile, line_d, line_edges, mirror  # noqa: E402

CODE128 = 4                                               # bit 2 of ``symbologies``
DEFAULTS = dict(symbologies=CODE128, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
ROW = 128                                                 # bytes of a result row
FNC1, FNC2, FNC3, FNC4 = 0xF1, 0xF2, 0xF3, 0xF4           # text elements beside the ASCII codes 0..127
START_A, START_B, START_C, STOP = 103, 104, 105, 106
MAX_VALUES = 62                                           # start + 60 data + check

# run widths for the values 0..106, a bar first; 103 / 104 / 105 are Start A / B / C, 106 is the first six runs of the stop
PATTERNS = [tuple(int(ch) for ch in s) for s in """
212222 222122 222221 121223 121322 131222 122213 122312 132212 221213 221312 231212 112232 122132 122231 113222 123122 123221 223211 221132
221231 213212 223112 312131 311222 321122 321221 312212 322112 322211 212123 212321 232121 111323 131123 131321 112313 132113 132311 211313
231113 231311 112133 112331 132131 113123 113321 133121 313121 211331 231131 213113 213311 213131 311123 311321 331121 312113 312311 332111
314111 221411 431111 111224 111422 121124 121421 141122 141221 112214 112412 122114 122411 142112 142211 241211 221114 413111 241112 134111
111242 121142 121241 114212 124112 124211 411212 421112 421211 212141 214121 412121 111143 111341 131141 114113 114311 411113 411311 113141
114131 311141 411131 211412 211214 211232 233111
""".split()]
KEYS = {tuple(n[k] + n[k + 1] for k in range(4)): v for v, n in enumerate(PATTERNS)}
assert len(PATTERNS) == 107 and len(set(PATTERNS)) == 107 and len(KEYS) == 107
assert all(sum(n) == 11 and min(n) >= 1 and max(n) <= 4 and (n[0] + n[2] + n[4]) % 2 == 0 for n in PATTERNS)


def decode_character(w6):
    """six run widths, a bar first -> the value 0..106 or None"""
    s = sum(w6)
    if s <= 0:
        return None
    key = tuple((22 * (w6[k] + w6[k + 1]) + s) // (2 * s) for k in range(4))
    if not all(2 <= e <= 7 for e in key) or key not in KEYS:
        return None
    value = KEYS[key]
    n = PATTERNS[value]
    if not 2 * abs(11 * (w6[0] + w6[2] + w6[4]) - s * (n[0] + n[2] + n[4])) < 3 * s:
        return None
    return value


def decode_candidate(e, l2d, i, quiet):
    """candidate start edge i -> the values [start, d_1 .. d_D, check] or None"""
    n = len(e)
    if not l2d[i] or i + 6 >= n:
        return None
    start = decode_character([e[i + k + 1] - e[i + k] for k in range(6)])
    if start not in (START_A, START_B, START_C):
        return None
    s_prev = e[i + 6] - e[i]
    if i >= 1 and 11 * (e[i] - e[i - 1]) < quiet * s_prev:
        return None
    values, j = [start], i + 6
    while True:
        if j + 6 >= n:
            return None
        s = e[j + 6] - e[j]
        if not 3 * s_prev <= 4 * s <= 5 * s_prev:
            return None
        v = decode_character([e[j + k + 1] - e[j + k] for k in range(6)])
        if v is None or v in (START_A, START_B, START_C):
            return None
        if v == STOP:
            break
        values.append(v)
        if len(values) > MAX_VALUES:
            return None
        s_prev, j = s, j + 6
    if j + 7 >= n:
        return None
    if (22 * (e[j + 7] - e[j + 6]) + s) // (2 * s) != 2:
        return None
    if j + 8 < n and 11 * (e[j + 8] - e[j + 7]) < quiet * s:
        return None
    if len(values) < 3:
        return None
    total = values[0] + sum(k * d for k, d in enumerate(values[1:-1], start=1))
    return values if total % 103 == values[-1] else None


def line_votes(e, l2d, w, quiet):
    """one scan line -> [(direction bit, values tuple)]: per direction the valid candidate with the lowest start"""
    votes = []
    for bit, (ee, pp) in ((1, (e, l2d)), (2, mirror(e, l2d, w))):
        for i in range(len(ee)):
            values = decode_candidate(ee, pp, i, quiet)
            if values is not None:
                votes.append((bit, tuple(values)))
                break
    return votes


def text_elements(values):
    """[start, d_1 .. d_D, check] -> the text elements: ASCII codes 0..127 and FNC1..FNC4 (0xF1..0xF4)"""
    cur, shift, out = "ABC"[values[0] - START_A], False, []
    for v in values[1:-1]:
        if cur == "C":
            if v < 100:
                out += [48 + v // 10, 48 + v % 10]
            elif v == 102:
                out.append(FNC1)
            else:
                cur = "B" if v == 100 else "A"
            continue
        code = ("B" if cur == "A" else "A") if shift else cur          # a shifted character is read in the other set
        shift = False
        if v < 96:
            out.append((v + 32 if v < 64 else v - 64) if code == "A" else v + 32)
        elif v == 96:
            out.append(FNC3)
        elif v == 97:
            out.append(FNC2)
        elif v == 98:
            shift = True
        elif v == 99:
            cur = "C"
        elif v == 100:
            if code == "A":
                cur = "B"
            else:
                out.append(FNC4)
        elif v == 101:
            if code == "A":
                out.append(FNC4)
            else:
                cur = "A"
        else:
            out.append(FNC1)
    return out


def none_row():
    return [0] * 8 + [0xFF] * (ROW - 8)


def tally(votes, min_votes):
    """all votes of a patch -> the result row of 128 bytes"""
    count, mask = {}, {}
    for bit, values in votes:
        count[values] = count.get(values, 0) + 1
        mask[values] = mask.get(values, 0) | bit
    if not count:
        return none_row()
    top = max(count.values())
    winners = [k for k, v in count.items() if v == top]
    if top < min_votes or len(winners) != 1:
        return none_row()
    values = list(winners[0])
    text = text_elements(values)
    head = [128, top, mask[winners[0]], len(text), 1 if values[1] == 102 else 0, len(values) - 2, values[0], values[-1]]
    return head + text + [0xFF] * (ROW - 8 - len(text))


def decode_patch(patch, symbologies=CODE128, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2):
    assert symbologies == CODE128
    lum = luma(patch)
    w = lum.shape[1]
    votes = []
    for k in range(scan_rows):
        p, m = line_profile(lum, k, scan_rows, band)
        e, l2d = line_edges(line_d(p, m, window, contrast))
        votes += line_votes(e, l2d, w, quiet)
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
