"""Test symbols for the two-width decoder: an encoder of Interleaved 2 of 5 and Code 39 from tables of its own (the public
nine-bit words of Code 39, ISO/IEC 16388, the most significant bit the first bar, 1 = wide; the weights 1 2 4 7 0 of ITF,
ISO/IEC 16390), independent of the pattern strings of tests/width_decode_oracle.py.  A symbol is a module string in units of
half a narrow run by default (narrow = 2 units), so that a wide run of 2, 2.5 or 3 narrow widths (4, 5, 6 units) is drawable;
the strings are drawn by text_decode_cases.render_modules and flat_row_modules."""
import numpy as np

import text_decode_cases as tc

C39_CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%*"           # a character's index is its check value; '*' is start and stop
C39_WORDS = [0x034, 0x121, 0x061, 0x160, 0x031, 0x130, 0x070, 0x025, 0x124, 0x064, 0x109, 0x049, 0x148, 0x019, 0x118, 0x058, 0x00D, 0x10C,
             0x04C, 0x01C, 0x103, 0x043, 0x142, 0x013, 0x112, 0x052, 0x007, 0x106, 0x046, 0x016, 0x181, 0x0C1, 0x1C0, 0x091, 0x190, 0x0D0,
             0x085, 0x184, 0x0C4, 0x0A8, 0x0A2, 0x08A, 0x02A, 0x094]
ITF_WEIGHTS = (1, 2, 4, 7, 0)                                         # a digit is the sum of the weights of its two wide runs; 11 reads as 0


def c39_wide(ch):
    """the nine runs of a character, a bar first: True = wide"""
    word = C39_WORDS[C39_CHARS.index(ch)]
    return [bool(word >> (8 - k) & 1) for k in range(9)]


def itf_wide(digit):
    """the five runs of one colour for a digit: True = wide"""
    for a in range(5):
        for b in range(a + 1, 5):
            if (ITF_WEIGHTS[a] + ITF_WEIGHTS[b]) % 11 == digit:
                return [k in (a, b) for k in range(5)]
    raise ValueError(digit)


def c39_check(text):
    return C39_CHARS[sum(C39_CHARS.index(ch) for ch in text) % 43]


def itf_check(digits):
    """the GS1 check digit behind an odd number of digits (the digit next to it weighs 3)"""
    digits = [int(d) for d in digits]
    return (10 - sum(d * (3 if k % 2 == 0 else 1) for k, d in enumerate(reversed(digits))) % 10) % 10


def c39_runs(text, narrow=2, wide=5, gap=None):
    """'*' + text + '*' -> the run widths in units, a bar first, ``gap`` units (default: narrow) of space between characters"""
    out = []
    for k, ch in enumerate("*" + text + "*"):
        if k:
            out.append(narrow if gap is None else gap)
        out += [wide if f else narrow for f in c39_wide(ch)]
    return out


def itf_runs(digits, narrow=2, wide=5):
    """an even number of digits -> start (n n n n), the interleaved pairs, stop (W n n): the run widths in units, a bar first"""
    digits = [int(d) for d in digits]
    assert len(digits) % 2 == 0
    out = [narrow] * 4
    for a, b in zip(digits[0::2], digits[1::2]):
        for fa, fb in zip(itf_wide(a), itf_wide(b)):
            out += [wide if fa else narrow, wide if fb else narrow]
    return out + [wide, narrow, narrow]


def modules_of(runs):
    """run widths in units, a bar first -> the module string of 0 / 1 (no quiet zone)"""
    return "".join(("1" if k % 2 == 0 else "0") * int(w) for k, w in enumerate(runs))


def c39_modules(text, narrow=2, wide=5, gap=None):
    return modules_of(c39_runs(text, narrow, wide, gap))


def itf_modules(digits, narrow=2, wide=5):
    return modules_of(itf_runs(digits, narrow, wide))


def flat_patch(strings, px_per_module, height, width, start, gap=0, channels=1):
    """(height, width, channels) uint8: the module strings side by side on every row"""
    row = tc.flat_row_modules(strings, px_per_module, width, start, gap)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (height, width, channels)))


def render(mods, px_per_module, angle=0.0, **kw):
    """text_decode_cases.render_modules with a quiet zone of ten narrow runs of 2 units"""
    return tc.render_modules(mods, px_per_module, angle, margin_modules=kw.pop("margin_modules", 20), **kw)


def edges_from_runs(widths, unit=256, start=256 * 20, grow=0):
    """run widths in units -> edge positions in 1/256 pixel (``unit`` per unit); ``grow`` widens every bar by that much and
    narrows the spaces alike; the first edge goes from light to dark"""
    e, pos = [start - grow // 2], start
    for k, w in enumerate(widths):
        pos += w * unit
        e.append(pos + (grow // 2 if k % 2 == 0 else -(grow // 2)))
    return e
