"""CPU: the numpy restatement of ubd_decode_text_patches (tests/text_decode_oracle.py) on Code 128 symbols encoded by
tests/text_decode_cases.py from a table of its own and drawn flat or rendered (super-sampled, rotated, blurred, noisy, unevenly
lit) and cut out with the patch oracle; and everything of the binding that needs no GPU: every refusal of the C entry point
(validation comes before any launch), the registered signature, the record conversion, the seams refusing to run without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
import object_patches_oracle as opo  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import text_decode_oracle as to  # noqa: E402

NONE = [0] * 8 + [0xFF] * 120
TEXTS = [("UBD-4711/AMD", False), ("0109501101530003171407041012345", True), ("a\tB\x00c 20261020 Zz", False)]
ANGLES = [-33.0, 101.0, 7.0]


def _row(values, votes, mask):
    text = to.text_elements(values)
    return [128, votes, mask, len(text), int(values[1] == 102), len(values) - 2, values[0], values[-1]] + text + [0xFF] * (120 - len(text))


def test_the_table():
    """107 distinct rows, each of 11 modules in widths 1..4 with an even bar sum, 107 distinct (E1..E4) keys with every E in
    2..7; the encoder's own copy says the same"""
    p = to.PATTERNS
    assert len(p) == 107 and len(set(p)) == 107
    assert all(len(n) == 6 and sum(n) == 11 and set(n) <= {1, 2, 3, 4} and (n[0] + n[2] + n[4]) % 2 == 0 for n in p)
    keys = {tuple(n[k] + n[k + 1] for k in range(4)) for n in p}
    assert len(keys) == 107 and all(2 <= e <= 7 for key in keys for e in key)
    assert [tuple(int(ch) for ch in tc.WIDTHS[6 * v:6 * v + 6]) for v in range(107)] == p
    assert all(len(c) == 11 and c[0] == "1" and c[-1] == "0" for c in tc.CODES)
    assert p[106] == (2, 3, 3, 1, 1, 1) and len(tc.modules([104, 1, 105])) == 3 * 11 + 13 and len(tc.runs([104, 1, 105])) == 3 * 6 + 7


def test_the_published_check_vector():
    """Start A + "PJJ123C" has the check value 54"""
    values = tc.values_with_check(tc.START_A, [ord(ch) - 32 for ch in "PJJ123C"])
    assert values[0] == 103 and values[-1] == 54
    assert bytes(to.text_elements(values)) == b"PJJ123C"
    assert bytes(to.text_elements(tc.encode_text("PJJ123C"))) == b"PJJ123C"


@pytest.mark.parametrize("grow", [0, 200, -200])
def test_every_value_decodes_to_itself(grow):
    """exact widths and +-20 % of a module of uniform bar growth"""
    for value, n in enumerate(to.PATTERNS):
        w = [k * 1000 + (grow if i % 2 == 0 else -grow) for i, k in enumerate(n)]
        assert to.decode_character(w) == value
    assert to.decode_character([0] * 6) is None and to.decode_character([5000, 1000, 1000, 1000, 1000, 2000]) is None


def test_the_bar_sum_test_rejects_what_the_edge_distances_accept():
    """bars thinner by 0.3 module and spaces wider alike keep every E_k (sums of a bar and a space) but move the bar sum by
    0.9 module of the allowed 1.5; by 0.55 module it is 1.65 and the character is gone"""
    n = to.PATTERNS[35]
    for shrink, want in ((300, 35), (550, None)):
        assert to.decode_character([k * 1000 + (-shrink if i % 2 == 0 else shrink) for i, k in enumerate(n)]) == want


def test_text_of_every_set_switch_and_shift():
    A, B, C = 103, 104, 105
    el = lambda start, data: to.text_elements(tc.values_with_check(start, data))  # noqa: E731
    assert el(A, [33, 64, 95, 0, 63]) == [65, 0, 31, 32, 95]                     # set A: 0..63 -> 32..95, 64..95 -> 0..31
    assert el(B, [33, 64, 95, 0]) == [65, 96, 127, 32]
    assert el(C, [0, 99, 42]) == [48, 48, 57, 57, 52, 50]
    assert el(A, [96, 97, 101, 102]) == [0xF3, 0xF2, 0xF4, 0xF1] and el(B, [96, 97, 100, 102]) == [0xF3, 0xF2, 0xF4, 0xF1]
    assert el(A, [98, 65, 65]) == [97, 1] and el(B, [98, 65, 65]) == [1, 97]       # Shift: one character in the other set
    assert el(A, [33, 98]) == [65] and el(B, [98]) == []                         # a trailing Shift is dropped
    assert el(A, [100, 65, 101, 65, 99, 12, 100, 65, 99, 7, 101, 65]) == [97, 1, 49, 50, 97, 48, 55, 1]
    assert el(C, [102, 12, 102, 100, 102]) == [0xF1, 49, 50, 0xF1, 0xF1]
    for text, gs1 in TEXTS + [("12", False), ("1234x", False), ("x12345", False), ("\x01\x02ab\x03", False), ("ab" + tc.FNC1 + "12345678", False)]:
        values = tc.encode_text(text, gs1)
        assert "".join(chr(v) for v in to.text_elements(values)) == (tc.FNC1 if gs1 else "") + text, (text, values)
    assert tc.encode_text("0109501101530003", True)[:3] == [C, 102, 1]


@pytest.mark.parametrize("px", [1, 2, 3])
def test_flat_symbols_upright_and_half_turned(px):
    for text, gs1 in TEXTS:
        values = tc.encode_text(text, gs1)
        patch = tc.flat_patch([values], px, 16, 1024, 40)
        assert to.decode_patch(patch) == _row(values, 8, 1), text
        assert to.decode_patch(patch[::-1, ::-1]) == _row(values, 8, 2), text
        assert to.decode_patch(np.repeat(patch, 3, axis=2)) == _row(values, 8, 1)


@pytest.mark.parametrize("px", [2, 3])
def test_rendered_symbols_decode(px):
    """blurred, noisy, unevenly lit, at three angles; extracted to 64 x 512 with expand 1.25"""
    for (text, gs1), angle in zip(TEXTS, ANGLES):
        values = tc.encode_text(text, gs1)
        frame, quad = tc.render(values, px, angle, seed=5, **dc.HARD)
        q = dc.int_quad(quad)
        upright = opo.extract(frame[:, :, None], q, 64, 512, None, 1.25)[0]
        r = to.decode_patch(upright)
        assert r[1] >= 2 and r == _row(values, r[1], 1), (text, r[:8])
        turned = opo.extract(frame[:, :, None], q[4:] + q[:4], 64, 512, None, 1.25)[0]
        r = to.decode_patch(turned)
        assert r[1] >= 2 and r == _row(values, r[1], 2), (text, r[:8])


def test_noise_stripes_and_retail_symbols_give_none():
    """at min_votes 1 and without a quiet zone: a single accepted candidate anywhere would show"""
    rng = np.random.default_rng(17)
    loose = dict(min_votes=1, quiet=0)
    for _ in range(25):
        assert to.decode_patch(rng.integers(0, 256, (64, 256, 1), dtype=np.uint8), **loose) == NONE
    for _ in range(25):
        row, x, v = np.zeros(512, np.uint8), 0, 0
        while x < 512:
            w = int(rng.integers(1, 9))
            row[x:x + w] = 225 if v else 35
            x, v = x + w, 1 - v
        assert to.decode_patch(np.broadcast_to(row[None, :, None], (64, 512, 1)), **loose) == NONE
    for body in ([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3], [0, 3, 6, 0, 0, 0, 2, 9, 1, 4, 5, 2], [5, 5, 1, 2, 3, 4, 5], [9, 6, 3, 8, 5, 0, 7]):
        for px in (1, 2, 3):
            patch = dc.flat_patch([dc.with_check(body)], px, 16, 512, 30)
            assert to.decode_patch(patch, **loose) == NONE and to.decode_patch(patch[::-1, ::-1], **loose) == NONE


def test_check_value_quiet_zone_and_length():
    values = tc.encode_text("UBD-4711")
    bad = values[:-1] + [(values[-1] + 1) % 103]
    assert to.decode_patch(tc.flat_patch([values], 2, 16, 512, 30))[0] == 128
    assert to.decode_patch(tc.flat_patch([bad], 2, 16, 512, 30), min_votes=1) == NONE
    for side in ("before", "behind"):                                   # a dark bar two modules away (QZ = 3) rejects, four modules away not
        for gap, want in ((2, 0), (4, 128)):
            patch = tc.flat_patch([values], 2, 16, 512, 30).copy()
            x = 30 - 2 * gap - 6 if side == "before" else 30 + 2 * len(tc.modules(values)) + 2 * gap
            patch[:, x:x + 6] = 35
            assert to.decode_patch(patch)[0] == want, (side, gap)
    assert to.decode_patch(tc.flat_patch([values], 2, 16, 512, 30), quiet=16)[0] == 128      # no neighbouring edge: the border passes
    assert to.decode_patch(tc.flat_patch([[104, 70]], 2, 16, 512, 30), min_votes=1) == NONE  # start and check alone: D = 0
    rng = np.random.default_rng(3)
    sixty = tc.values_with_check(104, rng.integers(0, 96, 60))
    sixty_one = tc.values_with_check(104, rng.integers(0, 96, 61))
    assert to.decode_patch(tc.flat_patch([sixty], 1, 4, 1024, 20), scan_rows=1, min_votes=1) == _row(sixty, 1, 1)
    assert to.decode_patch(tc.flat_patch([sixty_one], 1, 4, 1024, 20), scan_rows=1, min_votes=1) == NONE


def test_votes_ties_and_the_lowest_start():
    a, b = tc.encode_text("FIRST-1"), tc.encode_text("SECOND2")
    pa, pb = tc.flat_patch([a], 2, 64, 512, 30), tc.flat_patch([b], 2, 64, 512, 30)
    assert to.decode_patch(np.concatenate([pa[:32], pb[32:]])) == NONE  # four lines each
    more = np.concatenate([pa[:40], pb[40:]])
    assert to.decode_patch(more) == _row(a, 5, 1) and to.decode_patch(more, min_votes=6) == NONE
    both = tc.flat_patch([a, b], 1, 8, 512, 40, gap=20)
    assert to.decode_patch(both, scan_rows=1, min_votes=1) == _row(a, 1, 1)
    assert to.decode_patch(both[::-1, ::-1], scan_rows=1, min_votes=1) == _row(a, 1, 2)
    assert to.tally([(1, (104, 1, 105)), (2, (104, 1, 105)), (1, (104, 2, 3))], 2)[:8] == [128, 2, 3, 1, 0, 1, 104, 105]
    assert to.tally([(1, (104, 1, 105)), (1, (104, 2, 3))], 1) == NONE and to.tally([], 1) == NONE


def _good_args():
    from ubdvss_amd import _lib
    params = _lib.UbdDecodeParams(4, 8, 1, 16, 24, 3, 2)
    fake = ctypes.c_void_p(0x1000)                                      # never dereferenced: every call below is refused before a launch
    return params, dict(patches=fake, counts=fake, n=2, cap=4, patch_h=64, patch_w=256, channels=3, params=ctypes.pointer(params),
                        results=fake, stream=None)


def test_every_refusal_of_the_entry_point():
    from ubdvss_amd import _lib
    lib = _lib.load()
    assert _lib.SIGNATURES["ubd_decode_text_patches"] == _lib.SIGNATURES["ubd_decode_patches"] and lib.ubd_abi_version() == 3
    _, good = _good_args()
    bad = [("patches", None, "patches"), ("counts", None, "counts"), ("params", None, "params"), ("results", None, "results"),
           ("results", ctypes.c_void_p(0x1002), "aligned"), ("n", 0, "n must"), ("n", -1, "n must"), ("cap", 0, "cap must"),
           ("patch_h", 0, "patch_h"), ("patch_h", 1025, "patch_h"), ("patch_w", 31, "patch_w"), ("patch_w", 1025, "patch_w"),
           ("channels", 0, "channels"), ("channels", 2, "channels"), ("channels", 4, "channels")]
    for name, value, word in bad:
        args = dict(good)
        args[name] = value
        assert lib.ubd_decode_text_patches(*args.values()) != 0, (name, value)
        msg = lib.ubd_last_error().decode()
        assert msg.startswith("ubd_decode_text_patches") and word in msg, (name, value, msg)
    fields = [("symbologies", (0, 1, 3, 5, 7, 8, -1)), ("scan_rows", (0, 33)), ("band", (-1, 9)), ("window", (0, 65)), ("contrast", (-1, 256)),
              ("quiet", (-1, 17)), ("min_votes", (0, 17))]
    for field, values in fields:
        for value in values:
            params, args = _good_args()
            setattr(params, field, value)
            assert lib.ubd_decode_text_patches(*args.values()) != 0, (field, value)
            msg = lib.ubd_last_error().decode()
            assert msg.startswith("ubd_decode_text_patches") and field in msg, (field, value, msg)
    _, args = _good_args()
    args.update(n=1 << 16, cap=1 << 15)
    assert lib.ubd_decode_text_patches(*args.values()) != 0 and "2^31" in lib.ubd_last_error().decode()
    params, args = _good_args()                                         # the retail entry point keeps refusing bit 2
    args["params"] = ctypes.pointer(_lib.UbdDecodeParams(4, 8, 1, 16, 24, 3, 2))
    assert lib.ubd_decode_patches(*args.values()) != 0 and lib.ubd_last_error().decode().startswith("ubd_decode_patches")


def test_python_seams():
    import torch
    import ubdvss_amd
    from ubdvss_amd import barcode_decoder as bd
    assert ubdvss_amd.CODE128 == bd.CODE128 == to.CODE128 == 4 and bd.DEFAULT_PARAMS["symbologies"] == 3
    assert dict(bd.DEFAULT_PARAMS, symbologies=4) == to.DEFAULTS
    assert ubdvss_amd.DecodedText._fields == ("symbology", "text", "votes", "upside_down", "gs1", "elements")
    plain, gs1 = tc.encode_text("ab" + tc.FNC1 + "c" + tc.FNC2 + "\t"), tc.encode_text("0112345678901231" + tc.FNC1 + "10AB", True)
    results = np.zeros((2, 3, 128), np.uint8)
    results[:, :, 8:] = 0xFF
    results[0, 0], results[1, 0], results[1, 2] = _row(plain, 6, 1), _row(gs1, 4, 2), _row(plain, 2, 3)
    records = ubdvss_amd.text_results_to_records(results, np.array([2, 5], np.int32))
    assert [len(r) for r in records] == [2, 3] and records[0][1] is None and records[1][1] is None
    assert records[0][0] == ubdvss_amd.DecodedText("Code 128", "ab\x1dc\t", 6, False, False, (97, 98, 0xF1, 99, 0xF2, 9))
    assert records[1][0].text == "0112345678901231\x1d10AB" and records[1][0].gs1 and records[1][0].upside_down
    assert records[1][0].elements[0] == 0xF1 and records[1][0].votes == 4 and not records[1][2].upside_down
    if torch.cuda.is_available():
        return                                                          # the GPU tests run the rest
    with pytest.raises(RuntimeError):
        ubdvss_amd.decode_text_patches_on_device(np.zeros((1, 1, 8, 32, 1), np.uint8), np.zeros(1, np.int32))
    with pytest.raises(RuntimeError):
        ubdvss_amd.ModelRunner(ubdvss_amd.NetConfig(grey=False)).predict_decoded(None, [np.zeros((8, 8, 3), np.uint8)], symbologies=7)
