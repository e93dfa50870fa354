"""CPU: the numpy restatement of ubd_decode_width_patches (tests/width_decode_oracle.py) on ITF and Code 39 symbols encoded by
tests/width_decode_cases.py from tables of its own and drawn flat or rendered (super-sampled, rotated, blurred, noisy, unevenly
lit) and cut out with the patch oracle; and everything of the binding that needs no GPU: every refusal of the C entry point
(validation comes before any launch), the registered signature, the record conversion, the seams refusing to run without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
import decode_oracle as do  # noqa: E402
import object_patches_oracle as opo  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import text_decode_oracle as to  # noqa: E402
import width_decode_cases as wc  # noqa: E402
import width_decode_oracle as wo  # noqa: E402

NONE = [0] * 8 + [0xFF] * 120
GTIN14, CODE39_TEXT = "15400141288763", "CODE 39R"
WIDTHS = [(2, 2.5), (2, 3), (3, 2), (3, 2.5), (3, 3)]                   # the acceptance set: narrow run in pixels, wide : narrow


def _row(code, text, votes, mask):
    elements = [ord(ch) for ch in text]
    return [code, votes, mask, len(elements), int(wo.check_holds(code, elements)), 0, 0, 0] + elements + [0xFF] * (120 - len(elements))


def _pattern(flags):
    return "".join("W" if f else "n" for f in flags)


def test_the_tables():
    """44 distinct Code 39 patterns of three wide runs, ten ITF patterns of two; the encoder's words say the same; the four
    patterns include/ubd.h spells out; '*' read backwards is not '*'"""
    p = wo.C39_PATTERNS
    assert len(p) == 44 and len(set(p.values())) == 44 and all(len(k) == 9 and k.count("W") == 3 and set(k) == {"n", "W"} for k in p)
    assert len(set(wo.ITF_PATTERNS)) == 10 and all(len(k) == 5 and k.count("W") == 2 for k in wo.ITF_PATTERNS)
    assert {_pattern(wc.c39_wide(ch)): ch for ch in wc.C39_CHARS} == p
    assert [_pattern(wc.itf_wide(d)) for d in range(10)] == wo.ITF_PATTERNS
    by_char = {ch: k for k, ch in p.items()}
    assert (by_char["1"], by_char["A"], by_char["*"], by_char["%"]) == ("WnnWnnnnW", "WnnnnWnnW", "nWnnWnWnn", "nnnWnWnWn")
    assert p.get(by_char["*"][::-1]) != "*"
    assert [wo.C39_VALUES[ch] for ch in "09AZ-. $/+%"] == [0, 9, 10, 35, 36, 37, 38, 39, 40, 41, 42] and "*" not in wo.C39_VALUES
    assert wc.C39_CHARS[:43] == "".join(sorted(wo.C39_VALUES, key=wo.C39_VALUES.get))


def test_the_two_check_vectors():
    """the GTIN-14 15400141288763 holds the modulo-10 check; "CODE 39" sums to 113, its check value is 27 = R"""
    assert wo.check_holds(wo.CODE_ITF, [ord(ch) for ch in GTIN14]) and not wo.check_holds(wo.CODE_ITF, [ord(ch) for ch in "15400141288764"])
    assert wc.itf_check(GTIN14[:-1]) == 3
    assert sum(wo.C39_VALUES[ch] for ch in "CODE 39") == 113 and wc.c39_check("CODE 39") == "R" and wo.C39_VALUES["R"] == 27
    assert wo.check_holds(wo.CODE_39, [ord(ch) for ch in "CODE 39R"]) and not wo.check_holds(wo.CODE_39, [ord(ch) for ch in "CODE 39S"])
    assert not wo.check_holds(wo.CODE_39, [ord("0")])                    # T >= 2
    assert wo.check_holds(wo.CODE_ITF, [48, 48]) and wo.check_holds(wo.CODE_39, [ord("7"), ord("7")])


@pytest.mark.parametrize("grow", [0, 200, -200])
@pytest.mark.parametrize("narrow,wide", [(3, 9), (2, 6)])
def test_every_character_and_every_pair_decodes_to_itself(narrow, wide, grow):
    """exact widths and 200/256 pixel of uniform bar growth or shrinkage, at narrow runs of 3 and 2 pixels and a ratio of 3.
    (What growth g the rule itself allows: in a Code 39 character whose bars are all narrow, a bar n + g must stay at or below
    the middle of n - g and W - g, so 4 g <= W - n: a whole pixel at these widths, 0.75 pixel at 2 and 5.)"""
    for ch in wc.C39_CHARS:
        w = [256 * (wide if f else narrow) + (grow if k % 2 == 0 else -grow) for k, f in enumerate(wc.c39_wide(ch))]
        got = wo.decode_character(w)
        assert got is not None and got[0] == ch and got[1] == sum(v for v, f in zip(w, wc.c39_wide(ch)) if not f), (ch, got)
    for a in range(10):
        for b in range(10):
            w = [256 * v + (grow if k % 2 == 0 else -grow) for k, v in enumerate(wc.itf_runs([a, b], narrow, wide)[4:14])]
            assert wo.decode_pair(w)[:2] == (a, b), (a, b)
    assert wo.decode_character([0] * 9) is None and wo.decode_pair([256] * 10) is None


def test_two_or_four_wide_runs_are_no_character():
    """a wide run drawn narrow, a narrow run drawn wide; and wide runs that are not clear of the narrow ones (less than 1.5 times)"""
    base = [10 if f else 4 for f in wc.c39_wide("K")]
    assert wo.decode_character(base)[0] == "K"
    two, four = list(base), list(base)
    two[base.index(10)] = 4
    four[base.index(4)] = 10
    assert wo.decode_character(two) is None and wo.decode_character(four) is None
    assert wo.classify(four)[0].count("W") == 4 and wo.classify(two)[0].count("W") == 2
    assert wo.decode_character([6 if f else 4 for f in wc.c39_wide("K")])[0] == "K"         # 2 * 6 >= 3 * 4
    assert wo.decode_character([23 if f else 16 for f in wc.c39_wide("K")]) is None        # 2 * 23 < 3 * 16
    pair = wc.itf_runs([3, 8], 4, 10)[4:14]
    assert wo.decode_pair(pair)[:2] == (3, 8)
    for k in (pair.index(10), pair.index(4)):                           # three wide bars or spaces; one
        bad = list(pair)
        bad[k] = 14 - bad[k]
        assert wo.decode_pair(bad) is None


@pytest.mark.parametrize("narrow,wide", [(2, 5), (2, 6), (3, 6), (3, 8), (3, 9)])
def test_flat_symbols_upright_and_half_turned(narrow, wide):
    for code, mods, text in ((25, wc.itf_modules(GTIN14, narrow, wide), GTIN14), (39, wc.c39_modules(CODE39_TEXT, narrow, wide), CODE39_TEXT),
                             (25, wc.itf_modules("123456", narrow, wide), "123456"), (39, wc.c39_modules("-", narrow, wide), "-")):
        patch = wc.flat_patch([mods], 1, 16, 640, 40)
        assert wo.decode_patch(patch) == _row(code, text, 8, 1), text
        assert wo.decode_patch(patch[::-1, ::-1]) == _row(code, text, 8, 2), text
        assert wo.decode_patch(np.repeat(patch, 3, axis=2)) == _row(code, text, 8, 1)
        assert wo.decode_patch(patch, symbologies=wo.ITF if code == 39 else wo.CODE39) == NONE


@pytest.fixture(scope="module")
def acceptance_frames():
    """both symbologies at the five widths, CLEAN and HARD, at 0 and +-2 degrees: (code, text, patch width, frame, quad)"""
    out = []
    for code, text, mk in ((25, GTIN14, wc.itf_modules), (39, CODE39_TEXT, wc.c39_modules)):
        for narrow_px, ratio in WIDTHS:
            mods = mk(text, 2, int(2 * ratio))                          # half-narrow units
            pw = min(1024, int(np.ceil(1.25 * len(mods) * narrow_px / 2.0 / 64.0)) * 64)
            for kind in (dc.CLEAN, dc.HARD):
                for angle in (0.0, 2.0, -2.0):
                    out.append((code, text, pw) + wc.render(mods, narrow_px / 2.0, angle, seed=5, **kind))
    return out


def test_the_acceptance_set_is_read_completely(acceptance_frames):
    """every one of the 120 patches (upright and half-turned, extracted with expand 1.25 at about the drawn scale) reads to what
    was drawn with at least min_votes votes, in the right direction, the check flag set: no allowance for misses"""
    assert len(acceptance_frames) == 60
    for code, text, pw, frame, quad in acceptance_frames:
        q = dc.int_quad(quad)
        for mask, qq in ((1, q), (2, q[4:] + q[:4])):
            r = wo.decode_patch(opo.extract(frame[:, :, None], qq, 64, pw, None, 1.25)[0])
            assert r[1] >= 2 and r == _row(code, text, r[1], mask) and r[4] == 1, (code, pw, mask, r[:8])


def test_noise_stripes_and_other_families_give_none():
    """at min_votes 1 and without a quiet zone: a single accepted candidate anywhere would show"""
    rng = np.random.default_rng(17)
    loose = dict(min_votes=1, quiet=0)
    for _ in range(25):
        assert wo.decode_patch(rng.integers(0, 256, (64, 256, 1), dtype=np.uint8), **loose) == NONE
    for _ in range(25):
        assert wo.decode_patch(dc._stripes(rng, 64, 512)[:, :, None], **loose) == NONE
    for body in ([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3], [0, 3, 6, 0, 0, 0, 2, 9, 1, 4, 5, 2], [5, 5, 1, 2, 3, 4, 5], [9, 6, 3, 8, 5, 0, 7]):
        for px in (1, 2, 3):
            patch = dc.flat_patch([dc.with_check(body)], px, 16, 512, 30)
            assert wo.decode_patch(patch, **loose) == NONE and wo.decode_patch(patch[::-1, ::-1], **loose) == NONE
    for text, gs1 in (("UBD-4711/AMD", False), ("0109501101530003171407041012345", True), ("a\tB\x00c 20261020 Zz", False)):
        for px in (1, 2, 3):
            patch = tc.flat_patch([tc.encode_text(text, gs1)], px, 16, 1024, 40)
            assert wo.decode_patch(patch, **loose) == NONE and wo.decode_patch(patch[::-1, ::-1], **loose) == NONE


def test_the_other_two_oracles_read_nothing_on_two_width_symbols():
    loose = dict(min_votes=1, quiet=0)
    for narrow, wide in ((2, 5), (2, 6), (3, 6), (3, 9), (1, 2), (1, 3)):
        for mods in (wc.itf_modules(GTIN14, narrow, wide), wc.c39_modules(CODE39_TEXT, narrow, wide), wc.c39_modules("$%+/.-", narrow, wide)):
            patch = wc.flat_patch([mods], 1, 16, 640, 40)
            for p in (patch, patch[::-1, ::-1]):
                assert do.decode_patch(p, **loose) == [0, 0, 0] + [-1] * 13
                assert to.decode_patch(p, **loose) == NONE


def _patch(runs_px, width=512, start=40, height=16):
    return np.broadcast_to(dc._row_from_pixel_runs(runs_px, width, start)[None, :, None], (height, width, 1))


def test_quiet_zone():
    """QZ = 3 narrow runs: a dark bar two narrow runs before or behind the symbol rejects it, four away not; the patch border passes"""
    for code, runs, text in ((25, wc.itf_runs("123456", 4, 10), "123456"), (39, wc.c39_runs("AB", 4, 10), "AB")):
        assert wo.decode_patch(_patch(runs), quiet=16) == _row(code, text, 8, 1)
        for gap, want in ((8, NONE), (16, _row(code, text, 8, 1))):
            assert wo.decode_patch(_patch([6, gap] + runs, start=20)) == want, (code, "before", gap)
            assert wo.decode_patch(_patch(runs + [gap, 6])) == want, (code, "behind", gap)
            assert wo.decode_patch(_patch([6, gap] + runs, start=20), quiet=0) == _row(code, text, 8, 1)


def test_gap_and_width_drift():
    """Code 39: a gap of 2.5 narrow runs reads, a gap wider than half a character (54 pixels) does not; both symbologies: a
    character or pair drawn 1.22 times as wide as the one before it ends the candidate"""
    assert wo.decode_patch(_patch(wc.c39_runs("AB", 4, 10, gap=10))) == _row(39, "AB", 8, 1)
    assert wo.decode_patch(_patch(wc.c39_runs("AB", 4, 10, gap=27))) == _row(39, "AB", 8, 1)
    assert wo.decode_patch(_patch(wc.c39_runs("AB", 4, 10, gap=28)), min_votes=1) == NONE
    runs = wc.c39_runs("AB", 4, 10)
    drift = runs[:20] + wc.c39_runs("AB", 5, 12)[20:]
    assert len(runs) == 39 and wo.decode_patch(_patch(drift), min_votes=1) == NONE
    slow = runs[:20] + wc.c39_runs("AB", 4, 11)[20:]                    # 57 : 54 is within 9 : 8
    assert wo.decode_patch(_patch(slow)) == _row(39, "AB", 8, 1)
    runs = wc.itf_runs("12345678", 4, 10)
    assert wo.decode_patch(_patch(runs)) == _row(25, "12345678", 8, 1)
    drift = runs[:24] + wc.itf_runs("12345678", 5, 12)[24:]
    assert wo.decode_patch(_patch(drift), min_votes=1) == NONE


def test_pair_count_and_data_before_stop():
    """two pairs are no symbol, three are; 30 pairs are read and 31 are not; a last pair that begins W n n, as the stop does, is
    data because it reads as a pair"""
    assert wo.decode_patch(_patch(wc.itf_runs("1234", 4, 10)), min_votes=1) == NONE
    assert wo.decode_patch(_patch(wc.itf_runs("123456", 4, 10))) == _row(25, "123456", 8, 1)
    runs = wc.itf_runs("123410", 4, 10)
    assert runs[-13:-10] == [10, 4, 4] == runs[-3:]
    assert wo.decode_patch(_patch(runs)) == _row(25, "123410", 8, 1)
    rng = np.random.default_rng(3)
    sixty, sixty_two = "".join(map(str, rng.integers(0, 10, 60))), "".join(map(str, rng.integers(0, 10, 62)))
    assert wo.decode_patch(wc.flat_patch([wc.itf_modules(sixty, 1, 2)], 1, 4, 1024, 20), scan_rows=1, min_votes=1) == _row(25, sixty, 1, 1)
    assert wo.decode_patch(wc.flat_patch([wc.itf_modules(sixty_two, 1, 2)], 1, 4, 1024, 20), scan_rows=1, min_votes=1) == NONE
    chars = "".join(wc.C39_CHARS[int(v)] for v in rng.integers(0, 43, 61))
    assert wo.decode_patch(wc.flat_patch([wc.c39_modules(chars[:60], 1, 2)], 1, 4, 1024, 10), scan_rows=1, min_votes=1) == _row(39, chars[:60], 1, 1)
    assert wo.decode_patch(wc.flat_patch([wc.c39_modules("", 1, 2)], 1, 4, 1024, 10), scan_rows=1, min_votes=1) == NONE
    e = wc.edges_from_runs(wc.c39_runs(chars, 1, 2), unit=256, start=2560)
    assert len(e) == 630 and wo.c39_candidate(e, [k % 2 == 0 for k in range(len(e))], 0, 3) is None


def test_votes_ties_and_the_lowest_start():
    a, b = wc.itf_modules("123456", 2, 5), wc.itf_modules("654321", 2, 5)
    c = wc.c39_modules("AB", 2, 5)
    pa, pb = wc.flat_patch([a], 1, 64, 512, 30), wc.flat_patch([b], 1, 64, 512, 30)
    assert wo.decode_patch(np.concatenate([pa[:32], pb[32:]])) == NONE  # four lines each
    more = np.concatenate([pa[:40], pb[40:]])
    assert wo.decode_patch(more) == _row(25, "123456", 5, 1) and wo.decode_patch(more, min_votes=6) == NONE
    both = wc.flat_patch([a, b], 1, 8, 512, 40, gap=20)
    assert wo.decode_patch(both, scan_rows=1, min_votes=1) == _row(25, "123456", 1, 1)
    assert wo.decode_patch(both[::-1, ::-1], scan_rows=1, min_votes=1) == _row(25, "123456", 1, 2)
    mixed = wc.flat_patch([a, c], 1, 8, 512, 40, gap=30)                 # one symbol of each symbology: eight votes each
    assert wo.decode_patch(mixed) == NONE
    assert wo.decode_patch(mixed, symbologies=wo.ITF) == _row(25, "123456", 8, 1) and wo.decode_patch(mixed, symbologies=wo.CODE39) == _row(39, "AB", 8, 1)
    one, other = tuple(b"12"), tuple(b"21")
    assert wo.tally([(1, 39, one), (2, 39, one), (1, 25, one)], 2)[:8] == [39, 2, 3, 2, 0, 0, 0, 0]       # the symbology is part of the payload
    assert wo.tally([(1, 25, one), (1, 25, other)], 1) == NONE and wo.tally([(1, 25, one), (1, 39, one)], 1) == NONE and wo.tally([], 1) == NONE


def _good_args():
    from ubdvss_amd import _lib
    params = _lib.UbdDecodeParams(24, 8, 1, 16, 24, 3, 2)
    fake = ctypes.c_void_p(0x1000)                                      # never dereferenced: every call below is refused before a launch
    return params, dict(patches=fake, counts=fake, n=2, cap=4, patch_h=64, patch_w=256, channels=3, params=ctypes.pointer(params),
                        results=fake, stream=None)


def test_every_refusal_of_the_entry_point():
    from ubdvss_amd import _lib
    lib = _lib.load()
    assert _lib.SIGNATURES["ubd_decode_width_patches"] == _lib.SIGNATURES["ubd_decode_text_patches"] and lib.ubd_abi_version() == 3
    _, good = _good_args()
    bad = [("patches", None, "patches"), ("counts", None, "counts"), ("params", None, "params"), ("results", None, "results"),
           ("results", ctypes.c_void_p(0x1002), "aligned"), ("n", 0, "n must"), ("n", -1, "n must"), ("cap", 0, "cap must"),
           ("patch_h", 0, "patch_h"), ("patch_h", 1025, "patch_h"), ("patch_w", 31, "patch_w"), ("patch_w", 1025, "patch_w"),
           ("channels", 0, "channels"), ("channels", 2, "channels"), ("channels", 4, "channels")]
    for name, value, word in bad:
        args = dict(good)
        args[name] = value
        assert lib.ubd_decode_width_patches(*args.values()) != 0, (name, value)
        msg = lib.ubd_last_error().decode()
        assert msg.startswith("ubd_decode_width_patches") and word in msg, (name, value, msg)
    fields = [("symbologies", (0, 1, 4, 7, 9, 32, -1)), ("scan_rows", (0, 33)), ("band", (-1, 9)), ("window", (0, 65)), ("contrast", (-1, 256)),
              ("quiet", (-1, 17)), ("min_votes", (0, 17))]
    for field, values in fields:
        for value in values:
            params, args = _good_args()
            setattr(params, field, value)
            assert lib.ubd_decode_width_patches(*args.values()) != 0, (field, value)
            msg = lib.ubd_last_error().decode()
            assert msg.startswith("ubd_decode_width_patches") and field in msg, (field, value, msg)
    _, args = _good_args()
    args.update(n=1 << 16, cap=1 << 15)
    assert lib.ubd_decode_width_patches(*args.values()) != 0 and "2^31" in lib.ubd_last_error().decode()
    for entry in ("ubd_decode_patches", "ubd_decode_text_patches"):     # the other two entry points keep refusing bits 3 and 4
        for value in (8, 16, 24):
            params, args = _good_args()
            params.symbologies = value
            assert getattr(lib, entry)(*args.values()) != 0 and lib.ubd_last_error().decode().startswith(entry)


def test_python_seams():
    import torch
    import ubdvss_amd
    from ubdvss_amd import barcode_decoder as bd
    assert (ubdvss_amd.ITF, ubdvss_amd.CODE39) == (bd.ITF, bd.CODE39) == (wo.ITF, wo.CODE39) == (8, 16) and bd.DEFAULT_PARAMS["symbologies"] == 3
    assert dict(bd.DEFAULT_PARAMS, symbologies=24) == wo.DEFAULTS
    assert ubdvss_amd.DecodedWidth._fields == ("symbology", "text", "votes", "upside_down", "checked")
    results = np.zeros((2, 3, 128), np.uint8)
    results[:, :, 8:] = 0xFF
    results[0, 0], results[1, 0], results[1, 2] = _row(25, GTIN14, 6, 1), _row(39, "CODE 39R", 4, 2), _row(39, "A-1 $", 2, 3)
    records = ubdvss_amd.width_results_to_records(results, np.array([2, 5], np.int32))
    assert [len(r) for r in records] == [2, 3] and records[0][1] is None and records[1][1] is None
    assert records[0][0] == ubdvss_amd.DecodedWidth("ITF", GTIN14, 6, False, True)
    assert records[1][0] == ubdvss_amd.DecodedWidth("Code 39", "CODE 39R", 4, True, True)
    assert records[1][2] == ubdvss_amd.DecodedWidth("Code 39", "A-1 $", 2, False, False)
    assert ubdvss_amd.DecodedText._fields == ("symbology", "text", "votes", "upside_down", "gs1", "elements")
    assert ubdvss_amd.DecodedBarcode._fields == ("symbology", "text", "votes", "upside_down", "is_upc_a")
    if torch.cuda.is_available():
        return                                                          # the GPU tests run the rest
    with pytest.raises(RuntimeError):
        ubdvss_amd.decode_width_patches_on_device(np.zeros((1, 1, 8, 32, 1), np.uint8), np.zeros(1, np.int32))
    with pytest.raises(RuntimeError):
        ubdvss_amd.ModelRunner(ubdvss_amd.NetConfig(grey=False)).predict_decoded(None, [np.zeros((8, 8, 3), np.uint8)], symbologies=31)
