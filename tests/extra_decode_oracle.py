"""Numpy restatement of the three symbologies that joined the patch decoders' families (include/ubd.h), written from the rules
and not from the kernels: UPC-E in the retail family (ubd_decode_patches, bit 6), Code 93 in the text family
(ubd_decode_text_patches, bit 7) and Codabar in the two-width family (ubd_decode_width_patches, bit 8).  What a family had
before comes from its own oracle (tests/decode_oracle.py, text_decode_oracle.py, width_decode_oracle.py): the scan front end, the
older symbologies' candidates, the character rules the new ones share.  Per family there is ``*_line_votes`` (one scan line),
``*_tally`` (all votes -> the result row), ``decode_*_patch`` and ``decode_*_patches``.  Everything is integer arithmetic on
Python integers (exact); divisions floor, and every dividend is non-negative.  tests/test_extra_decode_host.py pins it on
rendered symbols; the device is compared with it by tests/test_gpu_extra_decode.py with np.array_equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_oracle as do  # noqa: E402
import text_decode_oracle as to  # noqa: E402
import width_decode_oracle as wo  # noqa: E402

EAN13, EAN8, CODE128, ITF, CODE39 = 1, 2, 4, 8, 16         # bits 0..4 of ``symbologies``; bit 5 is unassigned
UPCE, CODE93, CODABAR = 64, 128, 256                       # bits 6..8
RETAIL_MASK, TEXT_MASK, WIDTH_MASK = EAN13 | EAN8 | UPCE, CODE128 | CODE93, ITF | CODE39 | CODABAR
DEFAULTS = dict(scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)

# ---------------------------------------------------------------------------------------------------------------- UPC-E
UPCE_CODE, UPCE_RUNS, UPCE_MODULES, UPCE_QUIET = 6, 33, 51, 5
# the parity words of number system 0 for the check digits 0..9 (number system 1: L and G swapped)
UPCE_WORDS = "GGGLLL GGLGLL GGLLGL GGLLLG GLGGLL GLLGGL GLLLGG GLGLGL GLGLLG GLLGLG".split()


def upce_expand(d):
    """the six digits of a UPC-E -> the ten digits between number system and check digit of its UPC-A number"""
    d1, d2, d3, d4, d5, d6 = d
    if d6 <= 2:
        return [d1, d2, d6, 0, 0, 0, 0, d3, d4, d5]
    if d6 == 3:
        return [d1, d2, d3, 0, 0, 0, 0, 0, d4, d5]
    if d6 == 4:
        return [d1, d2, d3, d4, 0, 0, 0, 0, 0, d5]
    return [d1, d2, d3, d4, d5, 0, 0, 0, 0, d6]


def upca_check(eleven):
    """the check digit of number system + ten digits: the places 1, 3, .. 11 weigh 3"""
    return (10 - (3 * sum(eleven[0::2]) + sum(eleven[1::2])) % 10) % 10


def upce_candidate(e, l2d, i, quiet, trailing=UPCE_QUIET):
    """candidate start edge i -> [number system, d1 .. d6, check digit] or None.  ``trailing``: the modules of quiet zone the
    rules demand behind the symbol whatever ``quiet`` says (the tests set 0 to show what the rule is for)"""
    n = len(e)
    if not l2d[i] or i + UPCE_RUNS >= n:
        return None
    st = e[i + UPCE_RUNS] - e[i]
    if st <= 0:
        return None
    if i >= 1 and UPCE_MODULES * (e[i] - e[i - 1]) < quiet * st:
        return None
    if i + UPCE_RUNS + 1 < n and UPCE_MODULES * (e[i + UPCE_RUNS + 1] - e[i + UPCE_RUNS]) < max(quiet, trailing) * st:
        return None
    w = [e[i + j + 1] - e[i + j] for j in range(UPCE_RUNS)]
    for j in list(range(3)) + list(range(27, 33)):
        if (2 * UPCE_MODULES * w[j] + st) // (2 * st) != 1:
            return None
    chars = [do.decode_character(w[3 + 4 * k:7 + 4 * k], "LG") for k in range(6)]
    if None in chars:
        return None
    word, digits = "".join(c[0] for c in chars), [c[1] for c in chars]
    swapped = word.translate(str.maketrans("LG", "GL"))
    if word in UPCE_WORDS:
        ns, check = 0, UPCE_WORDS.index(word)
    elif swapped in UPCE_WORDS:
        ns, check = 1, UPCE_WORDS.index(swapped)
    else:
        return None
    if upca_check([ns] + upce_expand(digits)) != check:
        return None
    return [ns] + digits + [check]


def _first(ee, pp, candidate, *args):
    for i in range(len(ee)):
        got = candidate(ee, pp, i, *args)
        if got is not None:
            return tuple(got)
    return None


def retail_line_votes(e, l2d, w, symbologies, quiet, trailing=UPCE_QUIET):
    """one scan line -> [(direction bit, result code, digits tuple)]: per (direction, symbology) the valid candidate with the lowest start"""
    votes = do.line_votes(e, l2d, w, symbologies & (EAN13 | EAN8), quiet)
    if symbologies & UPCE:
        for bit, (ee, pp) in ((1, (e, l2d)), (2, do.mirror(e, l2d, w))):
            got = _first(ee, pp, upce_candidate, quiet, trailing)
            if got is not None:
                votes.append((bit, UPCE_CODE, got))
    return votes


retail_tally = do.tally                                     # (code, digits) payloads; a UPC-E row holds eight digits

# -------------------------------------------------------------------------------------------------------------- Code 93
C93_CODE, C93_STAR, C93_MAX_VALUES = 93, 47, 62             # byte 0 of a result row; start / stop; 60 data + C + K
C93_PATTERNS = [tuple(int(ch) for ch in s) for s in """
131112 111213 111312 111411 121113 121212 121311 111114 131211 141111 211113 211212 211311 221112 221211 231111 112113 112212 112311 122112
132111 111123 111222 111321 121122 131121 212112 212211 211122 211221 221121 222111 112122 112221 122121 123111 121131 311112 311211 321111
112131 113121 211131 121221 312111 311121 122211 111141
""".split()]
C93_KEYS = {tuple(n[k] + n[k + 1] for k in range(4)): v for v, n in enumerate(C93_PATTERNS)}
C93_CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%"  # the values 0..42; 43..46 are the shifts ($) (%) (/) (+)
C93_SHIFTS = (0xE1, 0xE2, 0xE3, 0xE4)                       # their text elements


def c93_character(w6):
    """six run widths, a bar first -> the value 0..47 or None"""
    s = sum(w6)
    if s <= 0:
        return None
    key = tuple((18 * (w6[k] + w6[k + 1]) + s) // (2 * s) for k in range(4))
    if not all(2 <= v <= 5 for v in key) or key not in C93_KEYS:
        return None
    value = C93_KEYS[key]
    n = C93_PATTERNS[value]
    if not 2 * abs(9 * (w6[0] + w6[2] + w6[4]) - s * (n[0] + n[2] + n[4])) < 3 * s:
        return None
    return value


def c93_checks(data):
    """the data values -> (C, K)"""
    c = sum(v * (k % 20 + 1) for k, v in enumerate(reversed(data))) % 47
    k = sum(v * (q % 15 + 1) for q, v in enumerate(reversed(list(data) + [c]))) % 47
    return c, k


def c93_candidate(e, l2d, i, quiet):
    """candidate start edge i -> the values [d_1 .. d_D, C, K] or None"""
    n = len(e)
    if not l2d[i] or i + 6 >= n:
        return None
    if c93_character([e[i + k + 1] - e[i + k] for k in range(6)]) != C93_STAR:
        return None
    s_prev = e[i + 6] - e[i]
    if i >= 1 and 9 * (e[i] - e[i - 1]) < quiet * s_prev:
        return None
    values, j = [], i + 6
    while True:
        if j + 6 >= n:
            return None
        s = e[j + 6] - e[j]
        if not 3 * s_prev <= 4 * s <= 5 * s_prev:
            return None
        v = c93_character([e[j + k + 1] - e[j + k] for k in range(6)])
        if v is None:
            return None
        if v == C93_STAR:
            break
        if len(values) == C93_MAX_VALUES:
            return None
        values.append(v)
        s_prev, j = s, j + 6
    if j + 7 >= n:
        return None
    if (18 * (e[j + 7] - e[j + 6]) + s) // (2 * s) != 1:                # the termination bar
        return None
    if j + 8 < n and 9 * (e[j + 8] - e[j + 7]) < quiet * s:
        return None
    if len(values) < 3:
        return None
    return values if c93_checks(values[:-2]) == (values[-2], values[-1]) else None


def c93_elements(data):
    return [ord(C93_CHARS[v]) if v < 43 else C93_SHIFTS[v - 43] for v in data]


def text_line_votes(e, l2d, w, symbologies, quiet):
    """one scan line -> [(direction bit, code, values tuple)]"""
    votes = [(bit, 128, values) for bit, values in to.line_votes(e, l2d, w, quiet)] if symbologies & CODE128 else []
    if symbologies & CODE93:
        for bit, (ee, pp) in ((1, (e, l2d)), (2, do.mirror(e, l2d, w))):
            got = _first(ee, pp, c93_candidate, quiet)
            if got is not None:
                votes.append((bit, C93_CODE, got))
    return votes


def _winner(votes, min_votes):
    """[(bit, code, payload)] -> (code, payload, votes, mask) of the one payload with the most votes, or None"""
    count, mask = {}, {}
    for bit, code, payload in votes:
        key = (code, payload)
        count[key] = count.get(key, 0) + 1
        mask[key] = mask.get(key, 0) | bit
    if not count:
        return None
    top = max(count.values())
    winners = [k for k, v in count.items() if v == top]
    if top < min_votes or len(winners) != 1:
        return None
    return winners[0][0], winners[0][1], top, mask[winners[0]]


def text_tally(votes, min_votes):
    """all votes of a patch -> the result row of 128 bytes"""
    won = _winner(votes, min_votes)
    if won is None:
        return to.none_row()
    code, values, top, mask = won
    if code == 128:
        return to.tally([(mask & 1 or 2, values)] * (top - 1) + [(mask & 2 or 1, values)], 1)      # the Code 128 row, its text expanded
    data = list(values[:-2])
    return [C93_CODE, top, mask, len(data), 0, len(data), values[-2], values[-1]] + c93_elements(data) + [0xFF] * (120 - len(data))


# -------------------------------------------------------------------------------------------------------------- Codabar
CBR_CODE, CBR_MAX_DATA = 27, 60
CBR_CHARS = "0123456789-$:/.+ABCD"                         # a character's index is its value
CBR_MASKS = [0x03, 0x06, 0x09, 0x60, 0x12, 0x42, 0x21, 0x24, 0x30, 0x48, 0x0C, 0x18, 0x45, 0x51, 0x54, 0x15, 0x1A, 0x29, 0x0B, 0x0E]
CBR_PATTERNS = {"".join("W" if m >> (6 - k) & 1 else "n" for k in range(7)): ch for m, ch in zip(CBR_MASKS, CBR_CHARS)}


def cbr_colour(runs):
    """the bars or the spaces of a character -> their pattern string of n / W, or None.  The family's narrow / wide rule, and
    beside it: a colour whose greatest run is less than 1.5 times its least has no wide run"""
    c = wo.classify(runs)
    if c is not None:
        return c[0]
    return "n" * len(runs) if 2 * max(runs) < 3 * min(runs) else None


def cbr_character(w7):
    """seven run widths, a bar first -> (character, sum of the narrow runs, their number) or None"""
    bars, spaces = cbr_colour(w7[0::2]), cbr_colour(w7[1::2])
    if bars is None or spaces is None:
        return None
    pattern = "".join(b + s for b, s in zip(bars, spaces + " ")).strip()
    if pattern not in CBR_PATTERNS:
        return None
    return CBR_PATTERNS[pattern], sum(w for w, f in zip(w7, pattern) if f == "n"), pattern.count("n")


def cbr_candidate(e, l2d, i, quiet):
    """candidate start edge i -> the ASCII codes of all its characters, start and stop included, or None"""
    n = len(e)
    if not l2d[i] or i + 7 >= n:
        return None
    start = cbr_character(wo._widths(e, i, 7))
    if start is None or start[0] not in "ABCD":
        return None
    _, n_prev, c_prev = start
    s_prev = e[i + 7] - e[i]
    if i >= 1 and c_prev * (e[i] - e[i - 1]) < quiet * n_prev:
        return None
    text, j = [ord(start[0])], i + 8
    while True:
        if j + 7 >= n:
            return None
        g = e[j] - e[j - 1]
        if not (n_prev <= 2 * c_prev * g and 2 * g <= s_prev):         # the gap: half a mean narrow run .. half a character
            return None
        ch = cbr_character(wo._widths(e, j, 7))
        if ch is None:
            return None
        if not 3 * n_prev * ch[2] <= 4 * ch[1] * c_prev <= 5 * n_prev * ch[2]:     # mean narrow runs of neighbours: 3/4 .. 5/4
            return None
        s_prev, n_prev, c_prev = e[j + 7] - e[j], ch[1], ch[2]
        if ch[0] in "ABCD":
            text.append(ord(ch[0]))
            break
        if len(text) == CBR_MAX_DATA + 1:
            return None
        text.append(ord(ch[0]))
        j += 8
    if len(text) < 3:
        return None
    if j + 8 < n and c_prev * (e[j + 8] - e[j + 7]) < quiet * n_prev:
        return None
    return text


def cbr_check_holds(elements):
    return sum(CBR_CHARS.index(chr(v)) for v in elements) % 16 == 0


def width_line_votes(e, l2d, w, symbologies, quiet):
    """one scan line -> [(direction bit, code, elements tuple)]"""
    votes = wo.line_votes(e, l2d, w, symbologies & (ITF | CODE39), quiet)
    if symbologies & CODABAR:
        for bit, (ee, pp) in ((1, (e, l2d)), (2, do.mirror(e, l2d, w))):
            got = _first(ee, pp, cbr_candidate, quiet)
            if got is not None:
                votes.append((bit, CBR_CODE, got))
    return votes


def width_tally(votes, min_votes):
    """all votes of a patch -> the result row of 128 bytes"""
    won = _winner(votes, min_votes)
    if won is None:
        return wo.none_row()
    code, elements, top, mask = won
    holds = cbr_check_holds(elements) if code == CBR_CODE else wo.check_holds(code, elements)
    return [code, top, mask, len(elements), int(holds), 0, 0, 0] + list(elements) + [0xFF] * (120 - len(elements))


# --------------------------------------------------------------------------------------------------------- the families
FAMILIES = {"retail": (retail_line_votes, retail_tally, RETAIL_MASK, 16, np.int32),
            "text": (text_line_votes, text_tally, TEXT_MASK, 128, np.uint8),
            "width": (width_line_votes, width_tally, WIDTH_MASK, 128, np.uint8)}


def accepted(family, symbologies):
    mask = FAMILIES[family][2]
    return symbologies > 0 and symbologies & ~mask == 0


def scan_lines(patch, scan_rows, band, window, contrast):
    """the edge lists (e, l2d) of the patch's scan lines: the front end all families share"""
    lum = do.luma(patch)
    return [do.line_edges(do.line_d(*do.line_profile(lum, k, scan_rows, band), window, contrast)) for k in range(scan_rows)]


def decode_lines(family, lines, width, symbologies, quiet, min_votes):
    line_votes, tally = FAMILIES[family][:2]
    assert accepted(family, symbologies)
    votes = []
    for e, l2d in lines:
        votes += line_votes(e, l2d, width, symbologies, quiet)
    return tally(votes, min_votes)


def decode_patch(family, patch, symbologies, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2):
    patch = np.asarray(patch)
    return decode_lines(family, scan_lines(patch, scan_rows, band, window, contrast), patch.shape[1], symbologies, quiet, min_votes)


def decode_patches(family, patches, counts, fill, **params):
    """(n, cap, h, w, c) uint8, counts (n) -> (n, cap, 16) int32 or (n, cap, 128) uint8; rows of slots j >= min(counts[i], cap) keep ``fill``"""
    patches = np.asarray(patches)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, FAMILIES[family][3]), fill, FAMILIES[family][4])
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            out[i, j] = decode_patch(family, patches[i, j], **params)
    return out
