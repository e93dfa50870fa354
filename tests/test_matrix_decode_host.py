"""CPU: the numpy restatement of ubd_decode_matrix_patches (tests/matrix_decode_oracle.py) on rendered Data Matrix symbols
(tests/matrix_decode_cases.py: an encoder with tables of its own and a renderer), the checks that hold without a second source
(the worked example of ISO/IEC 16022, the placement as a bijection, the codeword counts), Reed-Solomon at and beyond its limit,
and the host side of the Python layer (records, constants, the launch sets).  tests/test_gpu_matrix_decode.py holds the device
to the oracle on patches of the same set.

The acceptance set: nine texts, one per size, with digit pairs, upper shift, a first and a later FNC1; each at 4 pixels per
module (all sizes) and at 3 (sizes up to 22), in the four quarter turns, at 0, +-1 and +-2 degrees, clean and degraded (Gaussian
blur 0.7, a 25 % illumination ramp, noise sigma 5), in 128 x 128 patches: 640 patches, and the condition is zero misses."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
import matrix_decode_cases as mc  # noqa: E402
import matrix_decode_oracle as mo  # noqa: E402
import postal_decode_cases as pc  # noqa: E402
from ubdvss_amd import barcode_decoder as bd  # noqa: E402

NONE128 = list(mo.NONE)
# size -> (text, gs1): digit pairs everywhere, upper shift at 16 and 24, FNC1 first at 14, first and later at 18 and 26
TEXTS = {10: ("123456", False), 12: ("AB12", False), 14: ("011234", True), 16: ("Ubd-2026\xe9", False),
         18: ("10AB\x1d2112345678", True), 20: ("DATA MATRIX 20x20 ok", False), 22: ("https://example.org/p?id=314159", False),
         24: ("\xc4\xd6\xdc upper shift 24x24 0123456789", False), 26: ("0109501101530003\x1d17260930\x1d10LOT42", True)}
ANGLES = (0, 1, -1, 2, -2)


def expected_head(n, turns):
    """what a row must say of the symbol of size n as drawn: [0..4], U, and the elements; [5] and [6] are the reading's own"""
    text, gs1 = TEXTS[n]
    return [68, n, turns, len(text), int(gs1)], 0, [ord(ch) for ch in text]


def reads_as_drawn(row, n, turns):
    head, u, elements = expected_head(n, turns)
    t = len(elements)
    return list(row[:5]) == head and row[7] == u and list(row[8:8 + t]) == elements and all(v == 255 for v in row[8 + t:])


def acceptance_set():
    """-> [(n, pixels per module, turns, angle, degraded, patch (128, 128, 1))], 640 members"""
    out = []
    for n in mc.SIZES:
        sym = mc.symbol(TEXTS[n][0], n, TEXTS[n][1])
        for ppm in (4, 3) if n <= 22 else (4,):
            for turns in range(4):
                for angle in ANGLES:
                    for degraded in (False, True):
                        patch = mc.render(sym, ppm, angle=angle, turns=turns, seed=1 + len(out) % 3, **(mc.DEGRADED if degraded else {}))
                        out.append((n, ppm, turns, angle, degraded, patch))
    return out


@pytest.fixture(scope="module")
def acceptance_patches():
    return acceptance_set()


def test_the_worked_example_of_the_standard():
    """GF(256) with 0x12D and the roots a^1..a^5: "123456" is 142 164 186 and its check codewords 114 25 5 88 102"""
    assert mc.codewords("123456") == [142, 164, 186]
    assert mc.check_codewords([142, 164, 186], 5) == [114, 25, 5, 88, 102]
    assert mo.syndromes([142, 164, 186, 114, 25, 5, 88, 102], 5) == [0] * 5
    assert mo.reed_solomon([142, 164, 186, 114, 25, 5, 88, 102], 5) == ([142, 164, 186, 114, 25, 5, 88, 102], 0)
    assert mc.padded([66, 67, 142], 12) == [66, 67, 142, 129, 129 + (149 * 5) % 253 + 1 - 254]


def test_the_placement_is_a_bijection_with_the_four_fixed_corners():
    for n in mc.SIZES:
        m, total = n - 2, sum(mc.CAPACITY[n])
        pm = mc.placement(m)
        placed = sorted(int(v) for v in pm.ravel() if v >= 10)
        assert placed == [10 * ch + bit for ch in range(1, total + 1) for bit in range(1, 9)], n
        rest = [(r, c) for r in range(m) for c in range(m) if pm[r, c] < 10]
        if n in (12, 16, 20, 24):
            assert rest == [(m - 2, m - 2), (m - 2, m - 1), (m - 1, m - 2), (m - 1, m - 1)], n
            assert [int(pm[r, c]) for r, c in rest] == [1, 0, 0, 1]
        else:
            assert rest == [], n
        # and the oracle's walk undoes the encoder's map
        rng = np.random.default_rng(n)
        cws = [int(v) for v in rng.integers(0, 256, total)]
        assert mo.read_codewords(mc.symbol_from_codewords(cws, n).astype(bool)) == cws, n


def test_data_and_check_codewords_fill_the_mapping_matrix():
    assert mc.CAPACITY == mo.DATA_CHECK and tuple(mc.CAPACITY) == mc.SIZES == mo.SIZES == tuple(range(10, 27, 2))
    for n, (data, check) in mc.CAPACITY.items():
        assert data + check == (n - 2) ** 2 // 8, n
        assert len(mc.codewords(*TEXTS[n])) <= data, n
    assert sum(len(mc.codewords(*TEXTS[n])) < mc.CAPACITY[n][0] for n in mc.SIZES) >= 6    # the pad rule is exercised


def test_the_acceptance_set_has_640_patches(acceptance_patches):
    assert len(acceptance_patches) == 640
    assert all(m[5].shape == (128, 128, 1) and m[5].dtype == np.uint8 for m in acceptance_patches)
    assert {(m[0], m[1]) for m in acceptance_patches} == {(n, 4) for n in mc.SIZES} | {(n, 3) for n in mc.SIZES if n <= 22}


def test_the_oracle_reads_every_patch_of_the_acceptance_set(acceptance_patches):
    missed, most = [], 0
    for n, ppm, turns, angle, degraded, patch in acceptance_patches:
        row = mo.decode_patch(patch)
        if reads_as_drawn(row, n, turns):
            most = max(most, row[5])
        else:
            missed.append((n, ppm, turns, angle, degraded, row[:8]))
    print("most corrected codewords:", most)
    assert not missed, (len(missed), missed[:20])


@pytest.mark.parametrize("n", mc.SIZES)
def test_reed_solomon_at_and_beyond_its_limit(n):
    """exactly e / 2 corrupted codewords come back whole with corrected = e / 2; e / 2 + 1 read as none, on inputs chosen so
    that the oracle says none (a word that far off may lie within e / 2 of another codeword; such draws are passed over)"""
    data_n, e = mc.CAPACITY[n]
    data = mc.padded(mc.codewords(*TEXTS[n]), n)
    word = data + mc.check_codewords(data, e)
    rng = np.random.default_rng(100 + n)
    for _ in range(4):
        bad = list(word)
        for p in rng.choice(len(word), e // 2, replace=False):
            bad[p] ^= int(rng.integers(1, 256))
        assert mo.reed_solomon(bad, e) == (word, e // 2), n
    nones = 0
    for _ in range(8):
        bad = list(word)
        for p in rng.choice(len(word), e // 2 + 1, replace=False):
            bad[p] ^= int(rng.integers(1, 256))
        got = mo.reed_solomon(bad, e)
        assert got is None or (got[0] != word and not any(mo.syndromes(got[0], e))), n
        nones += got is None
    assert nones >= 4, n


def test_text_rules():
    assert mo.read_text([142, 164, 186]) == ([49, 50, 51, 52, 53, 54], 0, [])
    assert mo.read_text([232, 66, 232, 235, 106, 129, 70]) == ([65, 0x1D, 0xE9], 1, [])
    assert mo.read_text([66, 230, 1, 2]) == ([65], 2, [230, 1, 2])                  # C40 latch: the rest is raw
    assert mo.read_text([66, 235]) == ([65], 2, [235]) and mo.read_text([235, 200]) == ([], 2, [235, 200])
    assert mo.read_text([1, 128, 229]) == ([0, 127, 57, 57], 0, [])


def test_other_symbols_and_noise_read_as_none():
    rng = np.random.default_rng(11)
    stripes = dc._stripes(rng, 128, 128)[:, :, None]
    noise = rng.integers(0, 256, (128, 128, 1), dtype=np.uint8)
    ean = dc.flat_patch([dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])], 1, 128, 128, 10)
    rm = pc.render(pc.rm4scc_bars("SN34RD"), 4.0, 2.0, h=128, w=128)
    flat = np.full((128, 128, 1), 200, np.uint8)
    for patch in (stripes, noise, ean, rm, flat, np.zeros((32, 32, 1), np.uint8)):
        assert mo.decode_patch(patch) == NONE128
        assert mo.decode_patch(patch, contrast=0, band=0) == NONE128


def test_records_and_constants():
    assert bd.ALL_SYMBOLOGIES == 479 and bd.DATAMATRIX == 32768 == mo.DATAMATRIX == bd.MATRIX_SYMBOLOGIES and bd.MATRIX_RESULT_BYTES == 128
    assert not bd.MATRIX_SYMBOLOGIES & (bd.ALL_SYMBOLOGIES | bd.POSTAL_SYMBOLOGIES | 32 | 512 | 16384)
    rows = np.full((2, 2, 128), 0xA5, np.uint8)
    rows[0, 0] = mo.make_row(14, 3, 2, 1, [232, 66, 232, 235, 106, 142, 129, 70])
    rows[0, 1] = NONE128
    rows[1, 0] = mo.make_row(10, 0, 0, 0, [66, 230, 7])
    records = bd.matrix_results_to_records(rows, [2, 1])
    assert records == [[bd.DecodedMatrix("Data Matrix", "A\x1d\xe912", 14, 3, 2, True, True, b""), None],
                       [bd.DecodedMatrix("Data Matrix", "A", 10, 0, 0, False, False, bytes([230, 7]))]]
    assert bd.matrix_results_to_records(mo.decode_patches(np.zeros((1, 2, 32, 32, 1), np.uint8), [1], 0xA5), [1]) == [[None]]


def test_the_later_launched_set_is_the_headers():
    """as tests/test_postal_decode_host.py holds _lib.LAUNCHED: the entries whose last parameter is a `void *` under another name
    than `stream` or `hip_stream` that ends in `_stream` are exactly _lib.LAUNCHED_LATER, and that is the Data Matrix decoder"""
    from ubdvss_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ubd.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    entries = dict(re.findall(r"\b(ubd_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    any_stream = {name for name, params in entries.items() if re.search(r"\bvoid\s*\*\s*[a-z_]*stream\s*$", params.strip())}
    assert any_stream == _lib.LAUNCHED | _lib.LAUNCHED_LATER and not _lib.LAUNCHED & _lib.LAUNCHED_LATER
    assert _lib.LAUNCHED_LATER == {"ubd_decode_matrix_patches"} and isinstance(_lib.LAUNCHED_LATER, frozenset)
    assert re.search(r"\bvoid\s*\*\s*launch_stream\s*$", entries["ubd_decode_matrix_patches"].strip())
    assert not re.search(r"\d", "ubd_decode_matrix_patches")
    assert _lib.SIGNATURES["ubd_decode_matrix_patches"] == _lib.SIGNATURES["ubd_decode_postal_patches"]
    with pytest.raises(ValueError, match="ubd_decode_matrix_patches"):
        _lib.call("ubd_decode_matrix_patches", 1)
    with pytest.raises(ValueError, match="ubd_create"):
        _lib.launch("ubd_create", None)
