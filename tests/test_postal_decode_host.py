"""CPU: the numpy restatement of ubd_decode_postal_patches (tests/postal_decode_oracle.py) on rendered POSTNET, PLANET, RM4SCC and
KIX symbols (tests/postal_decode_cases.py: encoders with tables of their own and a 2-D renderer), and the host side of the
Python layer (records, kix_half_turned, the mask constants).  The acceptance set is chosen from what the oracle reads, and the
condition is zero misses; tests/test_gpu_postal_decode.py holds the device to the oracle on the same patches.

What the set holds: every kind at 2-pixel bars (pitch 5) and 3-pixel bars (pitch 6), clean and degraded (Gaussian blur 0.8 and
noise sigma 6), upright and half-turned, at 0 and +-1 degree, the 4-state kinds at +-2 degrees as well, scan_rows 16, in 64 x 256
patches or the narrowest wider one that holds the symbol.  Its limits, measured with the oracle while the set was chosen: at
2-pixel bars and pitch 4 (bars as wide as the gaps) the 2-state kinds stop reading under blur from 1 degree and the 4-state kinds
from 2 degrees; at pitch 4.5 and 5.5 single members of the sweep fail, at pitch 5 and at 3-pixel bars with pitch 6 or 7 none of
three noise seeds did; 3 degrees reads in part only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
import postal_decode_cases as pc  # noqa: E402
import postal_decode_oracle as po  # noqa: E402
import text_decode_cases as tc  # noqa: E402
from ubdvss_amd import barcode_decoder as bd  # noqa: E402

NONE128 = list(po.NONE)
POSTNET_ZIP, PLANET_DIGITS, RM_TEXT, KIX_TEXT = "801221905", "01234567890", "SN34RD1A", "2500GG30250"
DEGRADED = dict(blur=0.8, noise=6.0)
KINDS = {po.POSTNET: lambda: pc.postnet_bars(POSTNET_ZIP), po.PLANET: lambda: pc.planet_bars(PLANET_DIGITS),
         po.RM4SCC: lambda: pc.rm4scc_bars(RM_TEXT), po.KIX: lambda: pc.kix_bars(KIX_TEXT)}
TEXTS = {po.POSTNET: POSTNET_ZIP + str(pc.postnet_check(POSTNET_ZIP)), po.PLANET: PLANET_DIGITS + str(pc.postnet_check(PLANET_DIGITS)),
         po.RM4SCC: RM_TEXT + pc.rm4scc_check(RM_TEXT), po.KIX: KIX_TEXT}


def patch_width(n_bars, pitch, bar):
    """64 x 256 where the symbol fits with a pitch of margin on either side, else the narrowest wider multiple of 32"""
    w = 256
    while (n_bars + 1) * pitch + bar > w:
        w += 32
    return w


def expected_row(sym, text, votes, mask):
    n_bars = {po.POSTNET: 5 * len(text) + 2, po.PLANET: 5 * len(text) + 2, po.RM4SCC: 4 * len(text) + 2, po.KIX: 4 * len(text)}[sym]
    row = [po.CODES[sym], votes, mask, len(text), int(sym != po.KIX), n_bars, 0, 0] + [ord(ch) for ch in text]
    return row + [255] * (128 - len(row))


def acceptance_set():
    """-> [(symbology bit, the text it must read as, direction mask, patch (64, w, 1))], 128 members"""
    out = []
    for sym, bars in KINDS.items():
        bars = bars()
        for pitch, bar in ((5.0, 2.0), (6.0, 3.0)):
            w = patch_width(len(bars), pitch, bar)
            for degraded in (False, True):
                for turned in (False, True):
                    for angle in (0, 1, -1) + ((2, -2) if sym in (po.RM4SCC, po.KIX) else ()):
                        patch = pc.render(bars, pitch, bar, w=w, angle=angle, turned=turned, seed=1 + len(out) % 3, **(DEGRADED if degraded else {}))
                        text, mask = TEXTS[sym], 2 if turned else 1
                        if sym == po.KIX and turned:                    # read as it lies
                            text, mask = bd.kix_half_turned(text), 1
                        out.append((sym, text, mask, patch))
    return out


@pytest.fixture(scope="module")
def acceptance_patches():
    return acceptance_set()


def read(patch, **kw):
    return po.decode_patch(patch, **dict(dict(scan_rows=16), **kw))


def test_the_encoders_know_the_public_examples():
    assert pc.rm4scc_check("SN34RD1A") == "K"
    assert pc.postnet_bars("5")[1:6] == "SLSLS" and pc.postnet_bars("0")[1:6] == "LLSSS" and pc.planet_bars("0")[1:6] == "SSLLL"
    assert pc.planet_bars(PLANET_DIGITS)[1:11] == "SSLLLLLLSS"          # digits 0 then 1: six tall bars in a row
    assert pc.rm4scc_bars("0")[:5] == "ATTFF" and pc.rm4scc_bars("0")[-1] == "F" and pc.kix_bars("1A") == "TDAFDADA"
    assert len(set(pc.FOUR_STATE)) == 36 and all(sorted(w.replace("F", "AD").replace("T", "")) == list("AADD") for w in pc.FOUR_STATE)


def test_the_acceptance_set_reads_as_drawn(acceptance_patches):
    """zero misses, each under its own bit and with at least two votes; every fourth member also under the full mask"""
    assert len(acceptance_patches) == 128
    misses = []
    for k, (sym, text, mask, patch) in enumerate(acceptance_patches):
        for symbologies in (sym,) + ((po.MASK,) if k % 4 == 0 else ()):
            row = read(patch, symbologies=symbologies)
            if row[1] < 2 or row != expected_row(sym, text, row[1], mask):
                misses.append((k, symbologies, patch.shape, row[:8]))
    assert not misses, misses


def test_sn34rd1a_has_the_check_character_k():
    row = read(pc.render(pc.rm4scc_bars("SN34RD1A"), 6.0, 2.6))
    assert row == expected_row(po.RM4SCC, "SN34RD1AK", row[1], 1) and row[1] >= 3


def test_every_character_and_every_digit_round_trips():
    for part in ("012345678", "9ABCDEFGH", "IJKLMNOPQ", "RSTUVWXYZ"):
        text = part + pc.rm4scc_check(part)
        row = read(pc.render(pc.rm4scc_bars(part), 5.0, 2.0))
        assert row == expected_row(po.RM4SCC, text, row[1], 1), part
        row = read(pc.render(pc.kix_bars(part), 5.0, 2.0), symbologies=po.KIX)
        assert row == expected_row(po.KIX, part, row[1], 1), part
    digits = "01234567895"
    row = read(pc.render(pc.postnet_bars(digits), 5.0, 2.0, w=352))
    assert row == expected_row(po.POSTNET, digits + str(pc.postnet_check(digits)), row[1], 1)
    digits = "9876543210123"
    row = read(pc.render(pc.planet_bars(digits), 5.0, 2.0, w=384))
    assert row == expected_row(po.PLANET, digits + str(pc.postnet_check(digits)), row[1], 1) and row[5] == 72
    for digits in ("80122", "801225"):                                   # the two short lengths: 32 and 37 bars
        row = read(pc.render(pc.postnet_bars(digits), 5.0, 2.0))
        assert row == expected_row(po.POSTNET, digits + str(pc.postnet_check(digits)), row[1], 1)


def test_a_corrupted_check_reads_as_none():
    wrong = str((pc.postnet_check(POSTNET_ZIP) + 1) % 10)
    assert read(pc.render(pc.postnet_bars(POSTNET_ZIP, check=wrong), 5.0, 2.0, w=288)) == NONE128
    assert read(pc.render(pc.planet_bars(PLANET_DIGITS, check=wrong), 5.0, 2.0, w=320)) == NONE128
    assert read(pc.render(pc.rm4scc_bars(RM_TEXT, check="L"), 5.0, 2.0), symbologies=po.RM4SCC | po.POSTNET | po.PLANET) == NONE128
    assert read(pc.render(pc.rm4scc_bars(RM_TEXT, check="K"), 5.0, 2.0), symbologies=po.RM4SCC)[0] == 82


def test_a_postnet_of_another_length_reads_as_none():
    bars = pc.postnet_bars("80122190")                                  # eight digits and a check digit: 47 bars
    assert len(bars) == 47 and read(pc.render(bars, 5.0, 2.0)) == NONE128


def test_postnet_and_planet_are_told_apart_by_the_mask():
    planet, postnet = pc.render(pc.planet_bars(PLANET_DIGITS), 5.0, 2.0, w=320), pc.render(pc.postnet_bars("01234567895"), 5.0, 2.0, w=320)
    assert read(planet, symbologies=po.POSTNET) == NONE128 and read(postnet, symbologies=po.PLANET) == NONE128
    assert read(planet, symbologies=po.PLANET)[0] == 76 and read(postnet, symbologies=po.POSTNET)[0] == 80
    assert read(planet, symbologies=po.POSTNET | po.PLANET)[0] == 76 and read(postnet, symbologies=po.POSTNET | po.PLANET)[0] == 80


def test_a_kix_and_its_half_turned_text_are_each_others_reading():
    other = bd.kix_half_turned(KIX_TEXT)
    assert other != KIX_TEXT and bd.kix_half_turned(other) == KIX_TEXT
    upright, turned = pc.render(pc.kix_bars(KIX_TEXT), 5.0, 2.0), pc.render(pc.kix_bars(KIX_TEXT), 5.0, 2.0, turned=True)
    assert np.array_equal(turned[:, :, 0], upright[::-1, ::-1, 0])
    row = read(upright)
    assert row == expected_row(po.KIX, KIX_TEXT, row[1], 1)
    row = read(turned)
    assert row == expected_row(po.KIX, other, row[1], 1)               # mask 1: a KIX is read as the patch lies
    row = read(pc.render(pc.kix_bars(other), 5.0, 2.0, turned=True))
    assert row == expected_row(po.KIX, KIX_TEXT, row[1], 1)
    with pytest.raises(ValueError):
        bd.kix_half_turned("25-00")


def test_six_tall_bars_in_a_row_read():
    """PLANET digits 0 then 1 are SSLLL LLLSS: a row re-centred on every window of bars would leave the short bars behind them"""
    for angle in (0, 1):
        row = read(pc.render(pc.planet_bars(PLANET_DIGITS), 5.0, 2.0, w=320, angle=angle), symbologies=po.PLANET)
        assert row == expected_row(po.PLANET, TEXTS[po.PLANET], row[1], 1)


def _full_chains(patch, n_bars, group):
    """the scan lines of the patch on which some start edge's chain holds n_bars bars, the row tracking after ``group`` bars"""
    g, lines = po.scan_lines(patch, 16, 1, 16, 24)
    hits = 0
    for r, e, l2d in lines:
        chains = [po.walk(g, r, e[i], e[i + 1], group, 16, 24) for i in range(len(e) - 1) if l2d[i]]
        hits += any(ch is not None and len(ch[0]) == n_bars for ch in chains)
    return hits


def test_a_slanted_symbol_reads_only_because_the_row_tracks():
    """a KIX of 24 characters at 2 degrees: over its 96 bars the tracker band drifts by more than its own height, so no fixed row
    meets every bar (a tracking row that never starts: G beyond the chain), and the clamped row follows it"""
    text = "1234AB5678CD9012EF3456GH"
    patch = pc.render(pc.kix_bars(text), 5.0, 2.0, w=512, angle=2)
    row = read(patch, symbologies=po.KIX)
    assert row == expected_row(po.KIX, text, row[1], 1)
    assert _full_chains(patch, 96, 4) >= 2 and _full_chains(patch, 96, 1000) == 0


def test_other_symbols_and_noise_read_as_none_at_the_defaults():
    rng = np.random.default_rng(11)
    ean = dc.flat_patch([dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])], 2, 64, 256, 30)
    c128 = tc.flat_patch([tc.encode_text("UBD1")], 2, 64, 256, 40)
    noise = rng.integers(0, 256, (64, 256, 1), dtype=np.uint8)
    stripes = dc._stripes(rng, 64, 256)[:, :, None]
    for patch in (ean, c128, noise, stripes, np.full((64, 256, 1), 200, np.uint8)):
        assert po.decode_patch(patch) == NONE128
        assert po.decode_patch(patch, scan_rows=16, min_votes=1) == NONE128


def test_records_and_constants():
    assert bd.ALL_SYMBOLOGIES == 479
    assert (bd.POSTNET, bd.PLANET, bd.RM4SCC, bd.KIX) == (1024, 2048, 4096, 8192) == (po.POSTNET, po.PLANET, po.RM4SCC, po.KIX)
    assert bd.POSTAL_SYMBOLOGIES == 15360 == po.MASK and bd.POSTAL_RESULT_BYTES == 128 and not bd.POSTAL_SYMBOLOGIES & (bd.ALL_SYMBOLOGIES | 32 | 512)
    rows = np.full((2, 3, 128), 0xA5, np.uint8)
    rows[0, 0] = expected_row(po.RM4SCC, "SN34RD1AK", 5, 2)
    rows[0, 1] = NONE128
    rows[1, 0] = expected_row(po.KIX, KIX_TEXT, 3, 1)
    rows[1, 1] = expected_row(po.POSTNET, TEXTS[po.POSTNET], 4, 3)
    rows[1, 2] = expected_row(po.PLANET, TEXTS[po.PLANET], 2, 1)
    records = bd.postal_results_to_records(rows, [2, 3])
    assert records == [[bd.DecodedPostal("RM4SCC", "SN34RD1AK", 5, True, True, 38), None],
                       [bd.DecodedPostal("KIX", KIX_TEXT, 3, False, False, 44), bd.DecodedPostal("POSTNET", "8012219052", 4, False, True, 52),
                        bd.DecodedPostal("PLANET", "012345678905", 2, False, True, 62)]]
    assert bd.postal_results_to_records(po.decode_patches(np.zeros((1, 2, 8, 32, 1), np.uint8), [1], 0xA5), [1]) == [[None]]
    assert bd.kix_half_turned("0") == "Z" and bd.kix_half_turned("") == "" and bd.kix_half_turned("2500GG30250") == "Z5HZN88ZZ5H"


def test_launched_is_the_headers_set_of_entries_that_end_in_a_stream():
    """_lib.LAUNCHED against include/ubd.h, as tests/test_lib_call_host.py holds _lib.ON_STREAM: every declaration whose last
    parameter is `void *stream` or `void *hip_stream`, and the one entry beyond ON_STREAM is the postal decoder"""
    import re
    from ubdvss_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ubd.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    entries = dict(re.findall(r"\b(ubd_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    last_is_stream = {name for name, params in entries.items() if re.search(r"\bvoid\s*\*\s*(hip_)?stream\s*$", params.strip())}
    assert _lib.LAUNCHED == last_is_stream and _lib.LAUNCHED - _lib.ON_STREAM == {"ubd_decode_postal_patches"}
    assert isinstance(_lib.LAUNCHED, frozenset) and _lib.LAUNCHED <= set(_lib.SIGNATURES)
    res, args = _lib.SIGNATURES["ubd_decode_postal_patches"]
    assert res is _lib._i and args[-1] is _lib._vp and (res, args) == _lib.SIGNATURES["ubd_decode_width_patches"]
    with pytest.raises(ValueError, match="ubd_decode_postal_patches"):
        _lib.call("ubd_decode_postal_patches", 1)
