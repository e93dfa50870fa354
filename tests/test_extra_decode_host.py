"""CPU: the numpy restatement of UPC-E, Code 93 and Codabar (tests/extra_decode_oracle.py) on symbols encoded by
tests/extra_decode_cases.py from tables of its own and drawn flat or rendered (super-sampled, rotated, blurred, noisy, unevenly
lit) and cut out with the patch oracle; the known answers of include/ubd.h; every accepted and refused ``symbologies`` value of
the three C entry points (validation comes before any launch); the records and the three host helpers."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
import decode_oracle as do  # noqa: E402
import extra_decode_cases as xc  # noqa: E402
import extra_decode_oracle as xo  # noqa: E402
import object_patches_oracle as opo  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import text_decode_oracle as to  # noqa: E402
import width_decode_cases as wc  # noqa: E402
import width_decode_oracle as wo  # noqa: E402

NONE16, NONE128 = [0, 0, 0] + [-1] * 13, [0] * 8 + [0xFF] * 120
UPCE_A, UPCE_B = xc.upce_digits(0, "123456"), xc.upce_digits(1, "654321")
C93_TEXT, CBR_A, CBR_B = "TEST93", "A40156B", "C1:/.+$-D"
LOOSE = dict(min_votes=1, quiet=0)


def retail_row(digits, votes, mask):
    return [6, votes, mask] + list(digits) + [-1] * 5


def c93_row(text, votes, mask):
    values = xc.c93_values(text)
    data = values[:-2]
    return [93, votes, mask, len(data), 0, len(data), values[-2], values[-1]] + xo.c93_elements(data) + [0xFF] * (120 - len(data))


def cbr_row(text, votes, mask):
    elements = [ord(ch) for ch in text]
    return [27, votes, mask, len(elements), int(xo.cbr_check_holds(elements)), 0, 0, 0] + elements + [0xFF] * (120 - len(elements))


def acceptance_set():
    """(family, bit, expected row builder, pixels per unit, module string): UPC-E of both number systems and a Code 93 at 2 and
    3 pixels per module; two Codabars (one with every three-wide character) at narrow runs of 2 and 3 pixels and the ratios 2,
    2.5 and 3 (half-narrow units)"""
    out = []
    for px in (2, 3):
        out.append(("retail", xo.UPCE, lambda v, m: retail_row(UPCE_A, v, m), px, xc.upce_modules(UPCE_A)))
        out.append(("retail", xo.UPCE, lambda v, m: retail_row(UPCE_B, v, m), px, xc.upce_modules(UPCE_B)))
        out.append(("text", xo.CODE93, lambda v, m: c93_row(C93_TEXT, v, m), px, xc.c93_modules(xc.c93_values(C93_TEXT))))
    for narrow_px in (2, 3):
        for ratio in (2, 2.5, 3):
            for text in (CBR_A, CBR_B):
                out.append(("width", xo.CODABAR, lambda v, m, text=text: cbr_row(text, v, m), narrow_px / 2.0, xc.cbr_modules(text, 2, int(2 * ratio))))
    return out


@pytest.fixture(scope="module")
def acceptance_patches():
    """every symbol of the acceptance set CLEAN and HARD at 0 and +-2 degrees, extracted upright and half-turned with expand 1.25
    into 64 x 256, or 64 x 384 where the symbol does not fit: (family, bit, row builder, direction mask, patch)"""
    out = []
    for family, bit, row, px, mods in acceptance_set():
        pw = 256 if 1.25 * len(mods) * px <= 256 else 384
        for kind in (dc.CLEAN, dc.HARD):
            for angle in (0.0, 2.0, -2.0):
                frame, quad = xc.render(mods, px, angle, seed=5, **kind)
                q = dc.int_quad(quad)
                for mask, qq in ((1, q), (2, q[4:] + q[:4])):
                    out.append((family, bit, row, mask, opo.extract(frame[:, :, None], qq, 64, pw, None, 1.25)[0]))
    return out


def test_the_acceptance_set_is_read_completely(acceptance_patches):
    """all 216 patches read to what was drawn with at least min_votes votes in the right direction, no allowance for misses; and
    each reads "none" under the other symbologies of its family"""
    assert len(acceptance_patches) == 216
    others = {"retail": 3, "text": 4, "width": 24}
    for family, bit, row, mask, patch in acceptance_patches:
        lines = xo.scan_lines(patch, 8, 1, 16, 24)
        r = xo.decode_lines(family, lines, patch.shape[1], bit, 3, 2)
        assert r[1] >= 2 and r == row(r[1], mask), (family, patch.shape, mask, r[:12])
        assert xo.decode_lines(family, lines, patch.shape[1], bit | others[family], 3, 2) == r
        assert xo.decode_lines(family, lines, patch.shape[1], others[family], 3, 2) in (NONE16, NONE128)
    print("acceptance patches read:", len(acceptance_patches))


def test_the_known_answers_of_upce():
    """0 123456 5 expands to 0 12345 00006 with the check digit 5; the four expansions; the twenty parity words are distinct, hold
    three G each, and the encoder's hexadecimal words say the same as the oracle's strings"""
    assert xo.upce_expand([1, 2, 3, 4, 5, 6]) == [1, 2, 3, 4, 5, 0, 0, 0, 0, 6] and xo.upca_check([0, 1, 2, 3, 4, 5, 0, 0, 0, 0, 6]) == 5
    assert UPCE_A == [0, 1, 2, 3, 4, 5, 6, 5]
    assert xo.upce_expand([1, 2, 3, 4, 5, 1]) == [1, 2, 1, 0, 0, 0, 0, 3, 4, 5] and xo.upce_expand([1, 2, 3, 4, 5, 3]) == [1, 2, 3, 0, 0, 0, 0, 0, 4, 5]
    assert xo.upce_expand([1, 2, 3, 4, 5, 4]) == [1, 2, 3, 4, 0, 0, 0, 0, 0, 5]
    for ns in (0, 1):
        for six in ("123456", "000000", "999999", "481273", "306174", "750002", "555551"):
            eight = xc.upce_digits(ns, six)
            assert [ns] + xo.upce_expand(eight[1:7]) == xc.upce_to_upca11(ns, six) and xo.upca_check(xc.upce_to_upca11(ns, six)) == eight[7]
    words = [int(w.replace("G", "1").replace("L", "0"), 2) for w in xo.UPCE_WORDS]
    assert words == xc.UPCE_PARITY == [0x38, 0x34, 0x32, 0x31, 0x2C, 0x26, 0x23, 0x2A, 0x29, 0x25]
    assert len(set(words) | {w ^ 63 for w in words}) == 20 and all(bin(w).count("1") == 3 for w in words)
    assert xo.UPCE_WORDS[1].translate(str.maketrans("LG", "GL")) == "LLGLGG" == do.PARITY_WORDS[1]     # the hazard: EAN-13 first digit 1


def test_the_known_answers_of_code_93():
    """"TEST93" has C = 41 (+) and K = 6; 48 patterns of nine modules and runs 1..4 with 48 distinct keys in 2..5; the encoder's
    string says the same; the weights cycle after 20 and 15"""
    values = xc.c93_values("TEST93")
    assert values[-2:] == [41, 6] and xo.C93_CHARS[41] == "+" and xo.c93_checks(values[:-2]) == (41, 6)
    p = xo.C93_PATTERNS
    assert len(p) == 48 == len(set(p)) == len(xo.C93_KEYS) and all(sum(n) == 9 and 1 <= min(n) and max(n) <= 4 for n in p)
    assert all(2 <= v <= 5 for key in xo.C93_KEYS for v in key)
    assert ["".join(map(str, n)) for n in p] == [xc.C93_WIDTHS[6 * v:6 * v + 6] for v in range(48)] and p[47] == (1, 1, 1, 1, 4, 1)
    assert xc.C93_ALPHABET[:43] == xo.C93_CHARS
    data = [1] * 22
    assert xo.c93_checks(data)[0] == (sum(range(1, 21)) + 1 + 2) % 47
    assert xc.c93_values("1" * 22)[-2:] == list(xo.c93_checks(data))
    for grow in (0, 150, -150):                                          # every character reads as itself, exact and with ink spread
        for px in (2, 3):
            for v, n in enumerate(p):
                w = [256 * px * m + (grow if k % 2 == 0 else -grow) for k, m in enumerate(n)]
                assert xo.c93_character(w) == v, (v, grow, px)
    assert xo.c93_character([1024, 256, 256, 256, 256, 256]) is None and xo.c93_character([0] * 6) is None           # 411111 is no character
    # a composition of 9 that is no character: the key of 121212 shifted by one module (212121 has the same sums) fails the bar sum
    assert xo.c93_character([256 * v for v in (1, 2, 1, 2, 1, 2)]) == 5 and xo.c93_character([256 * v for v in (2, 1, 2, 1, 2, 1)]) is None


def test_the_known_answers_of_codabar():
    """twenty distinct masks; two wide runs for digits, - and $, three for the rest; the encoder's words say the same; no start
    pattern read backwards is in the table"""
    masks = dict(zip(xo.CBR_CHARS, xo.CBR_MASKS))
    assert len(set(xo.CBR_MASKS)) == 20 and len(xo.CBR_PATTERNS) == 20
    assert all(bin(masks[ch]).count("1") == (2 if ch in "0123456789-$" else 3) for ch in xo.CBR_CHARS)
    assert {ch: int(w, 2) for ch, w in xc.CBR_WORDS.items()} == masks
    for ch in "ABCD":
        assert int(format(masks[ch], "07b")[::-1], 2) not in xo.CBR_MASKS
    for grow in (0, 150, -150):
        for narrow, wide in ((2, 4), (2, 5), (2, 6), (3, 6), (3, 9)):
            for ch in xo.CBR_CHARS:
                w = [256 * v + (grow if k % 2 == 0 else -grow) for k, v in enumerate(xc.cbr_runs(ch, narrow, wide))]
                got = xo.cbr_character(w)
                assert got is not None and got[0] == ch and got[2] == (5 if ch in "0123456789-$" else 4), (ch, grow, narrow, wide, got)
    assert xo.cbr_character([512] * 7) is None and xo.cbr_colour([512, 700, 512]) == "nnn" and xo.cbr_colour([512, 800, 512]) == "nWn"
    assert xo.cbr_colour([512, 768, 600]) is None                        # 1.5 times the least, but not clear of the greatest narrow
    assert xo.cbr_check_holds([ord(c) for c in "A1D"]) is False and xo.cbr_check_holds([ord(c) for c in "A40156B"]) is False
    assert xo.cbr_check_holds([ord(c) for c in "A0A"]) and sum(xo.CBR_CHARS.index(c) for c in "A0A") == 32


@pytest.mark.parametrize("px", [1, 2, 3])
def test_flat_symbols_both_directions_and_one_direction_only(px):
    """upright and half-turned; at quiet 0 and min_votes 1 a symbol read the wrong way would show: each of the three votes in one
    direction only (a UPC-E has guards of three and six runs, a Code 93 ends in its termination bar, no Codabar start reads backwards)"""
    cases = [("retail", xo.UPCE, xc.upce_modules(UPCE_A), lambda v, m: retail_row(UPCE_A, v, m)),
             ("retail", xo.UPCE, xc.upce_modules(UPCE_B), lambda v, m: retail_row(UPCE_B, v, m)),
             ("text", xo.CODE93, xc.c93_modules(xc.c93_values(C93_TEXT)), lambda v, m: c93_row(C93_TEXT, v, m)),
             ("text", xo.CODE93, xc.c93_modules(xc.c93_values("ab$cZd+ %")), lambda v, m: c93_row("ab$cZd+ %", v, m)),
             ("width", xo.CODABAR, xc.cbr_modules(CBR_A, 2, 5), lambda v, m: cbr_row(CBR_A, v, m)),
             ("width", xo.CODABAR, xc.cbr_modules(CBR_B, 2, 6), lambda v, m: cbr_row(CBR_B, v, m))]
    for family, bit, mods, row in cases:
        patch = xc.flat_patch([mods], px, 16, 1024 if px * len(mods) > 480 else 512)
        for p, mask in ((patch, 1), (patch[::-1, ::-1], 2), (np.repeat(patch, 3, axis=2), 1)):
            assert xo.decode_patch(family, p, bit) == row(8, mask), (family, mask)
            assert xo.decode_patch(family, p, bit, **LOOSE) == row(8, mask)
            assert xo.decode_patch(family, p, xo.FAMILIES[family][2]) == row(8, mask)
        for e, l2d in xo.scan_lines(patch, 2, 0, 16, 24):
            votes = xo.FAMILIES[family][0](e, l2d, patch.shape[1], bit, 0)
            assert [v[0] for v in votes] == [1], (family, votes)


def test_the_shifts_of_code_93_are_elements():
    row = xo.decode_patch("text", xc.flat_patch([xc.c93_modules(xc.c93_values("aAbBcCdD"))], 1, 8, 256), xo.CODE93)
    assert row[:6] == [93, 8, 1, 8, 0, 8] and row[8:16] == [0xE1, 65, 0xE2, 66, 0xE3, 67, 0xE4, 68]


def _edges_of(mods_px):
    """a module string drawn at one pixel per module -> the edge list of a scan line"""
    patch = xc.flat_patch([mods_px], 1, 4, 1024, start=40)
    return xo.scan_lines(patch, 1, 0, 16, 24)[0]


def test_an_ean13_whose_left_half_is_a_upce_stays_an_ean13():
    """first digit 1 has the parity LLGLGG, the word 0B of number system 1 (check digit 1); the digits are chosen so that the
    UPC-A check of the left half holds: without the five-module rule the UPC-E reader accepts it, with the rule it does not"""
    left = next(six for six in ([int(c) for c in f"{v:06d}"] for v in range(1000000)) if xo.upca_check([1] + xo.upce_expand(six)) == 1)
    ean = dc.with_check([1] + left + [3, 0, 0, 0, 0])                    # the right half begins with the digit 3: a bar of one module, a space of four (the default quiet of 3 passes it)
    patch = dc.flat_patch([ean], 2, 16, 256, 30)
    e, l2d = xo.scan_lines(patch, 1, 0, 16, 24)[0]
    assert xo.upce_candidate(e, l2d, 0, 3, trailing=0) == [1] + left + [1]
    assert xo.upce_candidate(e, l2d, 0, 0, trailing=0) == [1] + left + [1] and xo.upce_candidate(e, l2d, 0, 0) is None
    assert xo.decode_patch("retail", patch, 67) == [13, 8, 1] + ean and xo.decode_patch("retail", patch, 64, **LOOSE) == NONE16
    votes = []
    for ee, pp in xo.scan_lines(patch, 8, 1, 16, 24):
        votes += xo.retail_line_votes(ee, pp, 256, 67, 3, trailing=0)
    assert xo.retail_tally(votes, 2) == NONE16                           # eight votes each: what the rule is for


def test_quiet_zones_guards_and_limits():
    u = xc.upce_modules(UPCE_A)
    for lead, trail, want in ((3, 5, True), (2, 5, False), (3, 4, False), (0, 5, False)):
        row = xo.decode_patch("retail", xc.flat_patch(["1" + "0" * lead + u + "0" * trail + "1"], 2, 8, 256), xo.UPCE)
        assert (row == retail_row(UPCE_A, 8, 1)) == want, (lead, trail)
    assert xo.decode_patch("retail", xc.flat_patch(["10" + u + "00001"], 2, 8, 256), xo.UPCE, quiet=0) == NONE16      # five modules whatever quiet says
    assert xo.decode_patch("retail", xc.flat_patch(["10" + u + "000001"], 2, 8, 256), xo.UPCE, quiet=0) == retail_row(UPCE_A, 8, 1)
    bad = xc.upce_digits(0, "123456")
    bad[7] = 6
    assert xo.decode_patch("retail", xc.flat_patch([xc.upce_modules(bad)], 2, 8, 256), xo.UPCE, **LOOSE) == NONE16  # the parity word says 6, the number 5
    c = xc.c93_modules(xc.c93_values("AB"))
    for lead, trail, want in ((3, 3, True), (2, 3, False), (3, 2, False)):
        row = xo.decode_patch("text", xc.flat_patch(["1" + "0" * lead + c + "0" * trail + "1"], 2, 8, 256), xo.CODE93)
        assert (row == c93_row("AB", 8, 1)) == want, (lead, trail)
    assert xo.decode_patch("text", xc.flat_patch([c[:-1]], 2, 8, 256), xo.CODE93, **LOOSE) == NONE128                # no termination bar
    wrong = xc.c93_values("AB")
    wrong[-1] = (wrong[-1] + 1) % 47
    assert xo.decode_patch("text", xc.flat_patch([xc.c93_modules(wrong)], 2, 8, 256), xo.CODE93, **LOOSE) == NONE128
    wrong = xc.c93_values("AB")
    wrong[-2] = (wrong[-2] + 1) % 47
    assert xo.decode_patch("text", xc.flat_patch([xc.c93_modules(wrong)], 2, 8, 256), xo.CODE93, **LOOSE) == NONE128
    rng = np.random.default_rng(3)
    long = "".join(xc.C93_ALPHABET[int(v)] for v in rng.integers(0, 47, 61))
    one = dict(scan_rows=1, min_votes=1)
    assert xo.decode_patch("text", xc.flat_patch([xc.c93_modules(xc.c93_values(long[:60]))], 1, 4, 1024), xo.CODE93, **one) == c93_row(long[:60], 1, 1)
    assert xo.decode_patch("text", xc.flat_patch([xc.c93_modules(xc.c93_values(long))], 1, 4, 1024), xo.CODE93, **one) == NONE128
    assert xo.decode_patch("text", xc.flat_patch([xc.c93_modules(xc.c93_values("7"))], 1, 4, 256), xo.CODE93, **one) == c93_row("7", 1, 1)
    assert xo.decode_patch("text", xc.flat_patch([xc.c93_modules(xc.c93_values(""))], 1, 4, 256), xo.CODE93, **one) == NONE128
    b = xc.cbr_runs("A12B", 4, 10)
    flat = lambda runs, start=40: np.broadcast_to(dc._row_from_pixel_runs(runs, 512, start)[None, :, None], (16, 512, 1))  # noqa: E731
    assert xo.decode_patch("width", flat(b), xo.CODABAR) == cbr_row("A12B", 8, 1)
    for gap, want in ((8, NONE128), (16, cbr_row("A12B", 8, 1))):
        assert xo.decode_patch("width", flat([6, gap] + b, 20), xo.CODABAR) == want and xo.decode_patch("width", flat(b + [gap, 6]), xo.CODABAR) == want
    assert xo.decode_patch("width", flat(xc.cbr_runs("A12B", 4, 10, gap=1)), xo.CODABAR, **LOOSE) == NONE128         # less than half a narrow run
    assert xo.decode_patch("width", flat(xc.cbr_runs("A12B", 4, 10, gap=20)), xo.CODABAR) == cbr_row("A12B", 8, 1)
    assert xo.decode_patch("width", flat(xc.cbr_runs("A12B", 4, 10, gap=24)), xo.CODABAR, **LOOSE) == NONE128        # more than half a character
    drift = b[:16] + xc.cbr_runs("A12B", 6, 15)[16:]
    assert xo.decode_patch("width", flat(drift), xo.CODABAR, **LOOSE) == NONE128                                     # narrow runs 1.5 times those before
    assert xo.decode_patch("width", flat(xc.cbr_runs("AB", 4, 10)), xo.CODABAR, **LOOSE) == NONE128                  # a stop behind no data
    data = "".join(xo.CBR_CHARS[int(v)] for v in rng.integers(0, 16, 61))
    assert xo.decode_patch("width", xc.flat_patch([xc.cbr_modules("A" + data[:60] + "D", 1, 2)], 1, 4, 1024), xo.CODABAR, **one) == cbr_row("A" + data[:60] + "D", 1, 1)
    assert xo.decode_patch("width", xc.flat_patch([xc.cbr_modules("A" + data + "D", 1, 2)], 1, 4, 1024), xo.CODABAR, **one) == NONE128


def test_old_and_new_symbologies_do_not_read_each_other():
    """at min_votes 1 and without a quiet zone (Codabar: at the defaults) the new readers find nothing in the older symbols,
    noise and stripes, and the older readers nothing in the new symbols"""
    rng = np.random.default_rng(17)
    old = [dc.flat_patch([dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])], 2, 16, 512, 30), dc.flat_patch([dc.with_check([5, 5, 1, 2, 3, 4, 5])], 2, 16, 512, 30),
           tc.flat_patch([tc.encode_text("UBD-4711/AMD")], 2, 16, 512, 40), wc.flat_patch([wc.itf_modules("15400141288763", 2, 5)], 1, 16, 512, 40),
           wc.flat_patch([wc.c39_modules("CODE 39R", 2, 5)], 1, 16, 512, 40)]
    old += [rng.integers(0, 256, (64, 256, 1), dtype=np.uint8) for _ in range(8)] + [dc._stripes(rng, 64, 512)[:, :, None] for _ in range(8)]
    for patch in old:
        for p in (patch, patch[::-1, ::-1]):
            lines = xo.scan_lines(p, 8, 1, 16, 24)
            for family, bit in (("retail", xo.UPCE), ("text", xo.CODE93)):
                assert xo.decode_lines(family, lines, p.shape[1], bit, 0, 1) in (NONE16, NONE128), family
            # (Codabar has no check character that rejects: in noise a single line can hold a start, a character and a stop.
            # The quiet zones and min_votes are its protection, so it is held to "none" at the defaults)
            assert xo.decode_lines("width", lines, p.shape[1], xo.CODABAR, 3, 2) == NONE128
    new = [xc.flat_patch([xc.upce_modules(UPCE_A)], 2, 16, 512), xc.flat_patch([xc.c93_modules(xc.c93_values(C93_TEXT))], 2, 16, 512),
           xc.flat_patch([xc.cbr_modules(CBR_B, 2, 5)], 1, 16, 512)]
    for k, patch in enumerate(new):
        for p in (patch, patch[::-1, ::-1]):
            assert do.decode_patch(p, **LOOSE) == NONE16 and to.decode_patch(p, **LOOSE) == NONE128 and wo.decode_patch(p, **LOOSE) == NONE128
            lines = xo.scan_lines(p, 8, 1, 16, 24)
            for q, (family, bit) in enumerate((("retail", xo.UPCE), ("text", xo.CODE93), ("width", xo.CODABAR))):
                assert (xo.decode_lines(family, lines, p.shape[1], bit, 0, 1)[0] != 0) == (q == k)


def test_the_family_oracles_agree_with_the_older_oracles_on_the_older_masks():
    patches = [dc.flat_patch([dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])], 2, 16, 512, 30), tc.flat_patch([tc.encode_text("UBD-4711/AMD")], 2, 16, 512, 40),
               wc.flat_patch([wc.c39_modules("CODE 39R", 2, 5)], 1, 16, 512, 40), xc.flat_patch([xc.upce_modules(UPCE_A)], 2, 16, 512)]
    for p in patches:
        for s in (1, 2, 3):
            assert xo.decode_patch("retail", p, s) == do.decode_patch(p, symbologies=s)
        assert xo.decode_patch("text", p, 4) == to.decode_patch(p)
        for s in (8, 16, 24):
            assert xo.decode_patch("width", p, s) == wo.decode_patch(p, symbologies=s)


ACCEPTED = {"ubd_decode_patches": (1, 2, 3, 64, 65, 66, 67), "ubd_decode_text_patches": (4, 128, 132),
            "ubd_decode_width_patches": (8, 16, 24, 256, 264, 272, 280)}
REFUSED = {"ubd_decode_patches": (0, 4, -1, 8, 16, 24, 32, 68, 128, 256, 96, 131, 479),
           "ubd_decode_text_patches": (0, 1, 3, 5, 7, 8, -1, 16, 24, 32, 64, 129, 136, 164, 256, 479),
           "ubd_decode_width_patches": (0, 1, 4, 7, 9, 32, -1, 40, 64, 128, 288, 312, 512, 479)}


def test_every_accepted_and_refused_symbologies_value_of_the_entry_points():
    """a refusal names ``symbologies``; an accepted value passes that check and is refused by the next one (min_votes 0), so
    nothing is launched here"""
    from ubdvss_amd import _lib
    lib = _lib.load()
    assert lib.ubd_abi_version() == 3
    fake = ctypes.c_void_p(0x1000)                                      # never dereferenced
    for entry in ACCEPTED:
        for values, accepted in ((ACCEPTED[entry], True), (REFUSED[entry], False)):
            for value in values:
                params = _lib.UbdDecodeParams(value, 8, 1, 16, 24, 3, 0)
                assert getattr(lib, entry)(fake, fake, 2, 4, 64, 256, 3, ctypes.pointer(params), fake, None) != 0
                msg = lib.ubd_last_error().decode()
                assert msg.startswith(entry) and ("min_votes" if accepted else "symbologies") in msg, (entry, value, msg)
                family = {"ubd_decode_patches": "retail", "ubd_decode_text_patches": "text", "ubd_decode_width_patches": "width"}[entry]
                assert xo.accepted(family, value) == accepted or (family == "text" and value in (4, 128, 132)) == accepted


def test_records_and_constants():
    import ubdvss_amd
    from ubdvss_amd import barcode_decoder as bd
    assert (ubdvss_amd.UPCE, ubdvss_amd.CODE93, ubdvss_amd.CODABAR) == (bd.UPCE, bd.CODE93, bd.CODABAR) == (xo.UPCE, xo.CODE93, xo.CODABAR) == (64, 128, 256)
    assert bd.ALL_SYMBOLOGIES == 479 == 1 | 2 | 4 | 8 | 16 | 64 | 128 | 256 and bd.DEFAULT_PARAMS["symbologies"] == 3
    retail = np.zeros((1, 2, 16), np.int32)
    retail[0, 0] = retail_row(UPCE_A, 5, 2)
    assert ubdvss_amd.results_to_records(retail, [2])[0] == [ubdvss_amd.DecodedBarcode("UPC-E", "01234565", 5, True, False), None]
    text = np.array([[c93_row("AbC", 4, 1), NONE128]], np.uint8)
    assert ubdvss_amd.text_results_to_records(text, [2])[0] == [ubdvss_amd.DecodedText("Code 93", "A\xe2C", 4, False, False, (65, 0xE2, 67)), None]
    width = np.array([[cbr_row("A0A", 3, 3), cbr_row(CBR_A, 2, 2)]], np.uint8)
    assert ubdvss_amd.width_results_to_records(width, [2])[0] == [ubdvss_amd.DecodedWidth("Codabar", "A0A", 3, False, True),
                                                                  ubdvss_amd.DecodedWidth("Codabar", CBR_A, 2, True, False)]


def test_upce_to_upca():
    from ubdvss_amd import upce_to_upca
    assert upce_to_upca("01234565") == "012345000065" == upce_to_upca("123456")
    assert upce_to_upca("04252614") == "042100005264"                   # the textbook example: 425261 -> 0 42100 00526 4
    for ns in (0, 1):
        for six in ("000000", "999999", "481273", "306174", "750002", "555551", "120453"):
            eight = "".join(map(str, xc.upce_digits(ns, six)))
            assert upce_to_upca(eight) == "".join(map(str, xc.upce_to_upca11(ns, six))) + eight[7]
    for bad in ("01234566", "21234565", "1234", "12345a", "", "0123456"):
        with pytest.raises(ValueError):
            upce_to_upca(bad)


def test_full_ascii():
    from ubdvss_amd import full_ascii
    assert full_ascii("+C+O+D+E 39") == "code 39" and full_ascii("CODE 39") == "CODE 39"
    assert full_ascii("$A$Z%A%E%F%J%K%O%P%T%U%V%W%X%Y%Z") == "\x01\x1a\x1b\x1f;?[_{\x7f\x00@`\x7f\x7f\x7f"
    assert full_ascii("/A/B/C/D/E/F/G/H/I/J/K/L/O/Z") == "!\"#$%&'()*+,/:" and full_ascii("-.") == "-."
    assert full_ascii("+A+Z") == "az"
    for bad in ("/P", "/Y", "$1", "A$", "+", "%-", "+a"):
        assert full_ascii(bad) is None, bad
    assert full_ascii((0xE4, 65, 66, 0xE1, 90)) == "aB\x1a" and full_ascii("\xe4A$B") == "a$B" and full_ascii((36, 65)) == "$A"
    assert full_ascii((0xE3, 80)) is None and full_ascii((0xE1,)) is None and full_ascii((0xE2, 0xE2)) is None and full_ascii((0xF1,)) is None
    assert full_ascii("") == "" and full_ascii(()) == ""
    elements = xo.decode_patch("text", xc.flat_patch([xc.c93_modules(xc.c93_values("dUdBdD-9cC"))], 1, 8, 512), xo.CODE93)[8:18]
    assert full_ascii(elements) == "ubd-9#"


def test_code32_to_digits():
    from ubdvss_amd import code32_to_digits
    alphabet = "0123456789BCDFGHJKLMNPQRSTUVWXYZ"

    def encode(nine):
        n, s = int(nine), ""
        for _ in range(6):
            n, s = n // 32, alphabet[n % 32] + s
        return s
    assert code32_to_digits(encode("012345676")) == "012345676"         # the pharmacode printed as A012345676
    assert code32_to_digits(encode("012345677")) is None and code32_to_digits(encode("000000000")) == "000000000"
    assert code32_to_digits("ZZZZZZ") is None and code32_to_digits("0123A5") is None and code32_to_digits("01234") is None
    assert code32_to_digits("0123456") is None and code32_to_digits("01 345") is None


def test_python_seams_without_a_gpu():
    import torch
    import ubdvss_amd
    if torch.cuda.is_available():
        return                                                          # the GPU tests run the rest
    with pytest.raises(RuntimeError):
        ubdvss_amd.ModelRunner(ubdvss_amd.NetConfig(grey=False)).predict_decoded(None, [np.zeros((8, 8, 3), np.uint8)], symbologies=479)
