"""Numpy restatement of ubd_decode_postal_patches (include/ubd.h), written from its specification and not from the kernel: the
height-modulated postal codes POSTNET, PLANET, RM4SCC and KIX.  The scan front end (luma, scan lines, band profile, local
threshold, sub-pixel edges, the mirrored list) is that of tests/decode_oracle.py and only finds the start edges; from a start edge
a chain of bars is walked on single-row luma, each bar measured up and down its centre column, and the bars' extents are
classified per character.  Everything is integer arithmetic on Python integers (exact); divisions floor, and every dividend is
non-negative.  tests/test_postal_decode_host.py pins it on rendered symbols; the device is compared with ``decode_patches`` by
tests/test_gpu_postal_decode.py with np.array_equal."""
import numpy as np

import decode_oracle as do

POSTNET, PLANET, RM4SCC, KIX = 1024, 2048, 4096, 8192   # bits of ``symbologies``
MASK = POSTNET | PLANET | RM4SCC | KIX
CODES = {POSTNET: 80, PLANET: 76, RM4SCC: 82, KIX: 75}  # byte 0 of a result row
GROUP = {POSTNET: 5, PLANET: 5, RM4SCC: 4, KIX: 4}      # G: the bars of a character, and of the tracking row's memory
DEFAULTS = dict(symbologies=MASK, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
ROW = 128
MAX_BARS = 122
POSTNET_BARS, PLANET_BARS = (32, 37, 52, 62), (62, 72)
DIGIT_WORDS = "11000 00011 00101 00110 01001 01010 01100 10001 10010 10100".split()
FOUR_WORDS = "0011 0101 0110 1001 1010 1100".split()
ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
NONE = [0] * 8 + [255] * (ROW - 8)


def measure(g, r, xc, window, memo):
    """a bar's centre pixel -> (Lmin, Lmax, top, bot); ``memo`` keeps what chains from different start edges measure again"""
    key = (r, xc)
    if memo is None or key not in memo:
        h, w = len(g), len(g[0])
        seg = g[r][max(0, xc - window):min(w - 1, xc + window) + 1]
        lmin, lmax = min(seg), max(seg)
        thr = lmin + lmax
        top = bot = r
        if 2 * g[r][xc] < thr:
            while top > 0 and 2 * g[top - 1][xc] < thr:
                top -= 1
            while bot < h - 1 and 2 * g[bot + 1][xc] < thr:
                bot += 1
        if memo is None:
            return lmin, lmax, top, bot
        memo[key] = (lmin, lmax, top, bot)
    return memo[key]


def walk(g, r, s, t, group, window, contrast, memo=None):
    """The chain of bars from the bar [s, t] (1/256 pixel) on row r of the luma ``g`` (a list of rows of Python integers);
    ``memo``: a dict of this (g, window) for ``measure``.
    -> None for a chain of more than MAX_BARS bars, else (bars [(top, bot)], s_first, t_last, the row after the last bar, the last bar's thr)"""
    w = len(g[0])
    bars, s_first, t_last, thr_last = [], s, t, 0
    s_prev = p_prev = None
    while True:
        xc = (s + t + 256) // 512
        lmin, lmax, top, bot = measure(g, r, xc, window, memo)
        thr = lmin + lmax
        if lmax - lmin < contrast or not 2 * g[r][xc] < thr:
            break
        p = None
        if s_prev is not None:
            p = s - s_prev
            if 4 * (t - s) > 3 * p:
                break
            if p_prev is not None and not 3 * p_prev <= 4 * p <= 5 * p_prev:
                break
        if len(bars) + 1 >= group:                         # the tracking row: clamped into what the last G bars share
            last = (bars + [(top, bot)])[-group:]
            hi_top, lo_bot = max(b[0] for b in last), min(b[1] for b in last)
            if lo_bot < hi_top:
                break
            q = (lo_bot - hi_top) // 4
            r = min(max(r, hi_top + q), lo_bot - q)
        bars.append((top, bot))
        t_last, thr_last = t, thr
        if len(bars) > MAX_BARS:
            return None
        s_prev, p_prev = s, p
        row = g[r]                                          # the next bar, on the (moved) row with this bar's thr
        x0 = t // 256 + 1
        xs = None
        for x in range(x0, min(x0 + (window if p is None else (2 * p) // 256), w - 1)):
            d0, d1 = 2 * row[x] - thr, 2 * row[x + 1] - thr
            if d0 >= 0 > d1:
                xs, s = x, 256 * x + (256 * d0) // (d0 - d1)
                break
        if xs is None:
            break
        xt = None
        for x in range(xs + 1, min(xs + 1 + window, w - 1)):
            d0, d1 = 2 * row[x] - thr, 2 * row[x + 1] - thr
            if d0 < 0 <= d1:
                xt, t = x, 256 * x + (256 * -d0) // (d1 - d0)
                break
        if xt is None:
            break
    return bars, s_first, t_last, r, thr_last


def quiet_behind(g, r, t_last, thr, pixels):
    w = len(g[0])
    x0 = t_last // 256 + 1
    return all(2 * g[r][x] >= thr for x in range(x0, min(x0 + pixels, w)))


def long_bars(values, groups, tallest):
    """per bar: long or short among its group's values (``groups``: (first, last) bar index pairs that cover every bar)"""
    out = [False] * len(values)
    for first, last in groups:
        part = values[first:last + 1]
        lo, hi = min(part), max(part)
        if 5 * (hi - lo) >= tallest:
            for k in range(first, last + 1):
                out[k] = 2 * values[k] > lo + hi
    return out


def framed_groups(n_bars, size):
    """the characters of a framed symbol: the frame bars join the first and the last group"""
    n = (n_bars - 2) // size
    return [(1 + size * k - (k == 0), size * (k + 1) + (k == n - 1)) for k in range(n)]


def word(flags, first, size):
    return "".join("1" if f else "0" for f in flags[first:first + size])


def four_state_value(la, lc, first):
    wa, wc = word(la, first, 4), word(lc, first, 4)
    if wa not in FOUR_WORDS or wc not in FOUR_WORDS:
        return None
    return 6 * FOUR_WORDS.index(wa) + FOUR_WORDS.index(wc)


def judge(bars, sym):
    """the bars of a chain as one symbol of ``sym`` -> its text, or None"""
    n_bars = len(bars)
    tallest = max(bot - top + 1 for top, bot in bars)
    a, c = [-top for top, _ in bars], [bot for _, bot in bars]
    if sym in (POSTNET, PLANET):
        if n_bars not in (POSTNET_BARS if sym == POSTNET else PLANET_BARS):
            return None
        groups = framed_groups(n_bars, 5)
        la, lc = long_bars(a, groups, tallest), long_bars(c, groups, tallest)
        if any(lc) or not la[0] or not la[-1]:
            return None
        digits = []
        for k in range(len(groups)):
            w5 = word(la, 1 + 5 * k, 5)
            if sym == PLANET:
                w5 = "".join("1" if ch == "0" else "0" for ch in w5)
            if w5 not in DIGIT_WORDS:
                return None
            digits.append(DIGIT_WORDS.index(w5))
        return "".join(map(str, digits)) if sum(digits) % 10 == 0 else None
    if sym == RM4SCC:
        if n_bars % 4 != 2 or not 2 <= (n_bars - 2) // 4 <= 30:
            return None
        groups = framed_groups(n_bars, 4)
        la, lc = long_bars(a, groups, tallest), long_bars(c, groups, tallest)
        if not la[0] or lc[0] or not la[-1] or not lc[-1]:
            return None
        values = [four_state_value(la, lc, 1 + 4 * k) for k in range(len(groups))]
        if None in values:
            return None
        rows, cols = sum(v // 6 + 1 for v in values[:-1]) % 6, sum(v % 6 + 1 for v in values[:-1]) % 6
        if values[-1] != 6 * ((rows + 5) % 6) + (cols + 5) % 6:
            return None
        return "".join(ALPHABET[v] for v in values)
    if n_bars % 4 != 0 or not 4 <= n_bars // 4 <= 30:
        return None
    groups = [(4 * k, 4 * k + 3) for k in range(n_bars // 4)]
    la, lc = long_bars(a, groups, tallest), long_bars(c, groups, tallest)
    values = [four_state_value(la, lc, 4 * k) for k in range(len(groups))]
    return None if None in values else "".join(ALPHABET[v] for v in values)


def candidate(g, r, e, l2d, i, group, syms, window, contrast, quiet, memo=None):
    """start edge i of one reading direction (g, r, e, l2d are that direction's) -> {symbology bit: (text, bars)} over ``syms``"""
    if not l2d[i] or i + 1 >= len(e):
        return {}
    chain = walk(g, r, e[i], e[i + 1], group, window, contrast, memo)
    if chain is None or not chain[0]:
        return {}
    bars, s_first, t_last, r_end, thr = chain
    n_bars, st = len(bars), t_last - s_first
    if i >= 1 and (2 * n_bars - 1) * (e[i] - e[i - 1]) < quiet * st:
        return {}
    den = (2 * n_bars - 1) * 256
    if not quiet_behind(g, r_end, t_last, thr, (quiet * st + den - 1) // den):
        return {}
    out = {}
    for sym in syms:
        text = judge(bars, sym)
        if text is not None:
            out[sym] = (text, n_bars)
    return out


def scan_lines(patch, scan_rows, band, window, contrast):
    """-> (luma rows, [(row r_k, edges, polarities)] per scan line): the part that does not depend on the symbologies"""
    lum = do.luma(patch)
    lines = []
    for k in range(scan_rows):
        p, m = do.line_profile(lum, k, scan_rows, band)
        e, l2d = do.line_edges(do.line_d(p, m, window, contrast))
        lines.append((((2 * k + 1) * lum.shape[0]) // (2 * scan_rows), e, l2d))
    return [[int(v) for v in row] for row in lum], lines


def decode_lines(scanned, symbologies, window, contrast, quiet, min_votes):
    """``scan_lines``' result -> the result row of 128 integers"""
    g, lines = scanned
    h, w = len(g), len(g[0])
    turned = [row[::-1] for row in g[::-1]]                  # direction 1 is direction 0 on the half-turned patch
    votes, memo = [], ({}, {})
    for r, e, l2d in lines:
        for bit, (gg, rr, (ee, pp)) in ((1, (g, r, (e, l2d))), (2, (turned, h - 1 - r, do.mirror(e, l2d, w)))):
            for group in (5, 4):
                syms = [s for s in CODES if symbologies & s and GROUP[s] == group and not (s == KIX and bit == 2)]
                for i in range(len(ee)):
                    if not syms:
                        break
                    for sym, (text, n_bars) in candidate(gg, rr, ee, pp, i, group, syms, window, contrast, quiet, memo[bit - 1]).items():
                        votes.append((bit, sym, text, n_bars))
                        syms.remove(sym)
    count, mask = {}, {}
    for bit, sym, text, n_bars in votes:
        key = (sym, text, n_bars)
        count[key] = count.get(key, 0) + 1
        mask[key] = mask.get(key, 0) | bit
    if not count:
        return list(NONE)
    top = max(count.values())
    winners = [k for k, v in count.items() if v == top]
    if top < min_votes or len(winners) != 1:
        return list(NONE)
    sym, text, n_bars = winners[0]
    row = [CODES[sym], top, mask[winners[0]], len(text), int(sym != KIX), n_bars, 0, 0] + [ord(ch) for ch in text]
    return row + [255] * (ROW - len(row))


def decode_patch(patch, symbologies=MASK, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2):
    return decode_lines(scan_lines(patch, scan_rows, band, window, contrast), symbologies, window, contrast, quiet, min_votes)


def decode_patches(patches, counts, fill, **params):
    """(n, cap, h, w, c) uint8, counts (n) -> uint8 (n, cap, 128); rows of slots j >= min(counts[i], cap) keep ``fill``"""
    patches = np.asarray(patches)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, ROW), fill, np.uint8)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            out[i, j] = decode_patch(patches[i, j], **dict(DEFAULTS, **params))
    return out
