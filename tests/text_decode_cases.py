"""Test symbols for the text decoder: an encoder of Code 128 / GS1-128 from the public module patterns (ISO/IEC 15417; a copy of
its own, independent of the table of tests/text_decode_oracle.py), from (start, data values) and from text with an automatic
choice of the code sets, and a renderer that draws any module string into a frame with the model of tests/decode_cases.render
(super-sampled, rotated, optional blur, noise and illumination ramp) and returns the true corners of the bar area."""
import numpy as np

import decode_cases as dc

START_A, START_B, START_C = 103, 104, 105
SHIFT, CODE_C, FNC1_VALUE = 98, 99, 102
FNC1, FNC2, FNC3, FNC4 = "\xf1", "\xf2", "\xf3", "\xf4"     # stand-ins for the function characters in the text given to encode_text

# the 107 characters: six run widths each, a bar first, one digit per run, and from them the eleven modules, 1 = dark
# (value 106 is the stop without its final bar of two modules)
WIDTHS = ("212222222122222221121223121322131222122213122312132212221213221312231212112232122132122231113222123122123221223211221132"
          "221231213212223112312131311222321122321221312212322112322211212123212321232121111323131123131321112313132113132311211313"
          "231113231311112133112331132131113123113321133121313121211331231131213113213311213131311123311321331121312113312311332111"
          "314111221411431111111224111422121124121421141122141221112214112412122114122411142112142211241211221114413111241112134111"
          "111242121142121241114212124112124211411212421112421211212141214121412121111143111341131141114113114311411113411311113141"
          "114131311141411131211412211214211232233111")
CODES = ["".join(("1" if k % 2 == 0 else "0") * int(ch) for k, ch in enumerate(WIDTHS[6 * v:6 * v + 6])) for v in range(107)]


def check_value(start, data):
    return (start + sum(k * d for k, d in enumerate(data, start=1))) % 103


def values_with_check(start, data):
    data = [int(d) for d in data]
    return [start] + data + [check_value(start, data)]


def modules(values):
    """[start, data.., check] -> the modules of the symbol as a string of 0 / 1 (no quiet zone): 11 per value and 13 of the stop"""
    return "".join(CODES[v] for v in values) + CODES[106] + "11"


def runs(values):
    m = modules(values)
    out, n = [], 1
    for a, b in zip(m, m[1:]):
        if a == b:
            n += 1
        else:
            out.append(n)
            n = 1
    return out + [n]


def _value_in(ch, code):
    """the value of character ``ch`` in set 'A' or 'B', or None"""
    if ch == FNC1:
        return 102
    if ch == FNC2:
        return 97
    if ch == FNC3:
        return 96
    if ch == FNC4:
        return 101 if code == "A" else 100
    o = ord(ch)
    if code == "A":
        return o - 32 if 32 <= o < 96 else o + 64 if o < 32 else None
    return o - 32 if 32 <= o < 128 else None


def _digits_ahead(text, k):
    n = 0
    while k + n < len(text) and text[k + n].isdigit():
        n += 1
    return n


def encode_text(text, gs1=False):
    """text (ASCII 0..127 and the FNC stand-ins above) -> [start, data.., check]: set C for runs of at least four digits (an even
    number of them), a Shift for a single character of the other set, a switch otherwise; gs1 puts FNC1 first"""
    if gs1:
        text = FNC1 + text
    k = 1 if gs1 else 0
    lead = _digits_ahead(text, k)
    if lead >= 4 or (lead >= 2 and lead % 2 == 0 and k + lead == len(text)):
        cur = "C"
    else:
        first = next((ch for ch in text if _value_in(ch, "A") is None or _value_in(ch, "B") is None), " ")
        cur = "A" if _value_in(first, "B") is None else "B"
    start, data, k = {"A": START_A, "B": START_B, "C": START_C}[cur], [], 0
    while k < len(text):
        ch = text[k]
        if cur == "C":
            if ch == FNC1:
                data.append(102)
                k += 1
            elif _digits_ahead(text, k) >= 2:
                data.append(int(text[k:k + 2]))
                k += 2
            else:
                cur = "B" if _value_in(ch, "B") is not None else "A"
                data.append(100 if cur == "B" else 101)
            continue
        ahead = _digits_ahead(text, k)
        if ahead >= 4 and ahead % 2 == 0 or ahead >= 5:
            if ahead % 2:                                               # an odd run: its first digit stays in this set
                data.append(_value_in(ch, cur))
                k += 1
            data.append(CODE_C)
            cur = "C"
            continue
        v = _value_in(ch, cur)
        if v is not None:
            data.append(v)
            k += 1
            continue
        other = "B" if cur == "A" else "A"
        if k + 1 < len(text) and _value_in(text[k + 1], cur) is None or k + 1 == len(text):
            data.append(100 if cur == "A" else 101)                     # Code B in set A, Code A in set B
            cur = other
        else:
            data += [SHIFT, _value_in(ch, other)]
            k += 1
    return values_with_check(start, data)


def flat_row_modules(strings, px_per_module, width, start, gap=0, light=225, dark=35):
    """one uint8 row of ``width`` pixels: the module strings drawn upright side by side at whole pixels per module"""
    row = np.full(width, light, np.uint8)
    x = start
    for m in strings:
        for ch in m:
            if ch == "1":
                row[x:x + px_per_module] = dark
            x += px_per_module
        x += gap
    assert x - gap <= width
    return row


def flat_patch(symbols, px_per_module, height, width, start, gap=0, channels=1):
    """(height, width, channels) uint8: the symbols (value lists) side by side on every row"""
    row = flat_row_modules([modules(v) for v in symbols], px_per_module, width, start, gap)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (height, width, channels)))


def render_modules(mods, px_per_module, angle=0.0, aspect=0.3, margin_modules=14, supersample=4, blur=0.0, noise=0.0, ramp=0.0,
                   seed=0, light=225.0, dark=35.0):
    """decode_cases.render for an arbitrary module string: -> (frame (h, w) uint8, quad), the same drawing model, the same quad"""
    m = np.array([int(ch) for ch in mods], np.int64)
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
        img = dc._blur(img, blur)
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


def render(values, px_per_module, angle=0.0, **kw):
    return render_modules(modules(values), px_per_module, angle, **kw)
