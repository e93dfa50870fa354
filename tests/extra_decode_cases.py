"""Test symbols for UPC-E, Code 93 and Codabar: encoders from tables of their own, independent of those of
tests/extra_decode_oracle.py (UPC-E from the seven-module characters of tests/decode_cases.py and parity words in hexadecimal;
Code 93 from one string of run widths; Codabar from the public bar / space words, 1 = wide).  Every encoder gives a module string
of 0 / 1 without quiet zones, which text_decode_cases.flat_row_modules and render_modules draw."""
import numpy as np

import decode_cases as dc
import text_decode_cases as tc

# UPC-E: the parity word of number system 0 for the check digits 0..9, bit 5 = first character, 1 = set G
UPCE_PARITY = [0x38, 0x34, 0x32, 0x31, 0x2C, 0x26, 0x23, 0x2A, 0x29, 0x25]


def upce_to_upca11(ns, six):
    """number system and the six digits -> the eleven digits of the UPC-A number without its check digit (zero suppression undone)"""
    d = [int(v) for v in six]
    if d[5] in (0, 1, 2):
        body = d[0:2] + [d[5], 0, 0, 0, 0] + d[2:5]
    elif d[5] == 3:
        body = d[0:3] + [0, 0, 0, 0, 0] + d[3:5]
    elif d[5] == 4:
        body = d[0:4] + [0, 0, 0, 0, 0] + d[4:5]
    else:
        body = d[0:5] + [0, 0, 0, 0] + d[5:6]
    return [int(ns)] + body


def upce_digits(ns, six):
    """-> the eight digits of the symbol: number system, six digits, check digit (that of the UPC-A number, as an EAN-13 with a leading 0)"""
    return [int(ns)] + [int(v) for v in six] + [dc.check_digit([0] + upce_to_upca11(ns, six))]


def upce_modules(eight):
    """[number system, d1..d6, check] -> the 51 modules"""
    ns, six, check = int(eight[0]), [int(v) for v in eight[1:7]], int(eight[7])
    word = UPCE_PARITY[check] ^ (0x3F if ns else 0)
    chars = "".join((dc.G_CODES if word >> (5 - k) & 1 else dc.L_CODES)[d] for k, d in enumerate(six))
    return "101" + chars + "010101"


# Code 93: six run widths per value 0..47, a bar first; 47 is start / stop
C93_WIDTHS = ("131112111213111312111411121113121212121311111114131211141111211113211212211311221112221211231111112113112212112311122112"
              "132111111123111222111321121122131121212112212211211122211221221121222111112122112221122121123111121131311112311211321111"
              "112131113121211131121221312111311121122211111141")
C93_ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%abcd"       # a..d stand for the shifts ($) (%) (/) (+) in the text given to c93_values


def c93_values(text):
    """text over C93_ALPHABET -> the data values with the two check characters behind them"""
    data = [C93_ALPHABET.index(ch) for ch in text]
    for span in (20, 15):
        data.append(sum(v * (k % span + 1) for k, v in enumerate(reversed(data))) % 47)
    return data


def c93_modules(values):
    """[data.., C, K] -> start, the values, stop and the termination bar"""
    return "".join("".join(("1" if k % 2 == 0 else "0") * int(ch) for k, ch in enumerate(C93_WIDTHS[6 * v:6 * v + 6]))
                   for v in [47] + list(values) + [47]) + "1"


# Codabar: the seven runs of a character, a bar first, 1 = wide
CBR_WORDS = {"0": "0000011", "1": "0000110", "2": "0001001", "3": "1100000", "4": "0010010", "5": "1000010", "6": "0100001", "7": "0100100",
             "8": "0110000", "9": "1001000", "-": "0001100", "$": "0011000", ":": "1000101", "/": "1010001", ".": "1010100", "+": "0010101",
             "A": "0011010", "B": "0101001", "C": "0001011", "D": "0001110"}


def cbr_runs(text, narrow=2, wide=5, gap=None):
    """all characters of ``text`` (start and stop included) -> the run widths in units, ``gap`` units (default: narrow) between characters"""
    out = []
    for k, ch in enumerate(text):
        if k:
            out.append(narrow if gap is None else gap)
        out += [wide if f == "1" else narrow for f in CBR_WORDS[ch]]
    return out


def cbr_modules(text, narrow=2, wide=5, gap=None):
    return "".join(("1" if k % 2 == 0 else "0") * int(w) for k, w in enumerate(cbr_runs(text, narrow, wide, gap)))


def flat_patch(strings, px_per_module, height, width, start=None, gap=0, channels=1):
    """(height, width, channels) uint8: the module strings side by side on every row; ``start`` None centres them"""
    if start is None:
        start = (width - px_per_module * sum(len(m) for m in strings) - gap * (len(strings) - 1)) // 2
    row = tc.flat_row_modules(strings, px_per_module, width, start, gap)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (height, width, channels)))


def render(mods, px_per_module, angle=0.0, **kw):
    return tc.render_modules(mods, px_per_module, angle, **kw)
