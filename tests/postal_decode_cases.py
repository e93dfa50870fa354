"""Test inputs of the postal decoder: encoders of POSTNET, PLANET, RM4SCC and KIX with tables of their own (written from the
public descriptions of the codes, independently of tests/postal_decode_oracle.py's word lists), and a 2-D renderer that draws the bars
on a supersampled canvas.  A symbol is a string of bar states: of a 4-state code T (tracker), A (ascender), D (descender) and
F (full), with ascender : tracker : descender = 3 : 2 : 3; of a 2-state code L (tall) and S (short, 2 / 5 of the tall bar, on
the same base line)."""
import numpy as np

from decode_cases import _blur, _tint

POSTNET_WEIGHTS = (7, 4, 2, 1, 0)                       # a digit is the two weights that sum to it; 0 is 7 + 4
ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
FOUR_STATE = ("TTFF TDAF TDFA DTAF DTFA DDAA TADF TFTF TFDA DATF DADA DFTA TAFD TFAD TFFT DAAD DAFT DFAT "
              "ATDF ADTF ADDA FTTF FTDA FDTA ATFD ADAD ADFT FTAD FTFT FDAT AADD AFTD AFDT FATD FADT FFTT").split()
# the extent of a bar state as fractions of the symbol's height, from its centre line, downwards positive
EXTENT = {"T": (-0.125, 0.125), "A": (-0.5, 0.125), "D": (-0.125, 0.5), "F": (-0.5, 0.5), "L": (-0.5, 0.5), "S": (0.1, 0.5)}


def postnet_check(digits):
    return (10 - sum(int(d) for d in digits) % 10) % 10


def _two_of_five(digit):
    want = 11 if digit == 0 else digit
    pair = next((a, b) for k, a in enumerate(POSTNET_WEIGHTS) for b in POSTNET_WEIGHTS[k + 1:] if a + b == want)
    return "".join("L" if wt in pair else "S" for wt in POSTNET_WEIGHTS)


def postnet_bars(digits, check=None):
    """the digits (a str, without the check digit) -> L / S states: frame bar, five bars a digit, check digit, frame bar"""
    digits = str(digits) + str(postnet_check(digits) if check is None else check)
    return "L" + "".join(_two_of_five(int(d)) for d in digits) + "L"


def planet_bars(digits, check=None):
    """PLANET: POSTNET with every digit's bars inverted (three tall)"""
    inner = postnet_bars(digits, check)[1:-1]
    return "L" + "".join("S" if ch == "L" else "L" for ch in inner) + "L"


def rm4scc_check(text):
    rows = sum(ALPHABET.index(ch) // 6 + 1 for ch in text) % 6
    cols = sum(ALPHABET.index(ch) % 6 + 1 for ch in text) % 6
    return ALPHABET[((rows - 1) % 6) * 6 + (cols - 1) % 6]


def rm4scc_bars(text, check=None):
    """the characters (without the check character) -> T / A / D / F states: start bar A, the characters, the check, stop bar F"""
    text = text + (rm4scc_check(text) if check is None else check)
    return "A" + "".join(FOUR_STATE[ALPHABET.index(ch)] for ch in text) + "F"


def kix_bars(text):
    return "".join(FOUR_STATE[ALPHABET.index(ch)] for ch in text)


def render(bars, pitch, bar, h=64, w=256, angle=0.0, blur=0.0, noise=0.0, ramp=0.0, seed=0, turned=False, channels=1, height=0.8,
           supersample=4, light=225.0, dark=35.0):
    """(h, w, channels) uint8: the bar states ``bars`` drawn upright about the patch's centre at ``pitch`` pixels from bar to bar
    and ``bar`` pixels a bar, the symbol ``height`` of the patch high, rotated by ``angle`` degrees (clockwise on the screen),
    then Gaussian blur (sigma in pixels), an illumination ramp from left to right (1 -+ ramp), noise (sigma in grey levels),
    and at last the half turn.  channels = 3 tints the grey image (decode_cases._tint)."""
    width, high = (len(bars) - 1) * float(pitch) + bar, height * h
    assert width + 2 * pitch <= w, (width, w)
    t = np.deg2rad(angle)
    ct, st = np.cos(t), np.sin(t)
    xx = ((np.arange(w * supersample) + 0.5) / supersample - w / 2.0)[None, :]
    yy = ((np.arange(h * supersample) + 0.5) / supersample - h / 2.0)[:, None]
    u, v = ct * xx + st * yy + width / 2, (-st * xx + ct * yy) / high
    idx = np.clip(np.floor(u / pitch).astype(np.int64), 0, len(bars) - 1)
    up = np.array([EXTENT[ch][0] for ch in bars])[idx]
    down = np.array([EXTENT[ch][1] for ch in bars])[idx]
    ink = (u >= 0) & (u < width) & (u - idx * pitch < bar) & (v >= up) & (v <= down)
    img = np.where(ink, dark, light).reshape(h, supersample, w, supersample).mean(axis=(1, 3))
    if blur:
        img = _blur(img, blur)
    if ramp:
        img = img * (1.0 + ramp * (2.0 * np.arange(w) / (w - 1) - 1.0))[None, :]
    if noise:
        img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape)
    grey = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if turned:
        grey = grey[::-1, ::-1]
    return np.ascontiguousarray(_tint(grey, channels, seed=seed))
