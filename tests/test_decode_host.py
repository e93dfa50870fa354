"""CPU: the numpy restatement of ubd_decode_patches (tests/decode_oracle.py) on symbols encoded from the public 7-module tables
and rendered by tests/decode_cases.py (super-sampled, rotated, blurred, noisy, unevenly lit), cut out with the patch oracle
tests/object_patches_oracle.py; and everything of the binding that needs no GPU: every refusal of the C entry point (validation
comes before any launch), the registered signature, the Python seams refusing to run without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
import decode_oracle as do  # noqa: E402
import object_patches_oracle as opo  # noqa: E402

# an EAN-13, a UPC-A (first digit 0), an EAN-13 with a mixed parity word, an EAN-8; each with its angle in the frame
SYMBOLS = [dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3]), dc.with_check([0, 3, 6, 0, 0, 0, 2, 9, 1, 4, 5, 2]),
           dc.with_check([9, 7, 8, 1, 8, 6, 1, 9, 7, 2, 7, 1]), dc.with_check([5, 5, 1, 2, 3, 4, 5])]
ANGLES = [0.0, 7.5, -33.0, 101.0]


def _widths(code):
    """seven modules as a string -> the four run widths"""
    out, n = [], 1
    for a, b in zip(code, code[1:]):
        if a == b:
            n += 1
        else:
            out.append(n)
            n = 1
    return out + [n]


def _grown(widths, first_is_bar, grow, unit=1000):
    """run widths in modules -> in units, every bar wider by ``grow`` and every space narrower by it"""
    return [n * unit + (grow if (k % 2 == 0) == first_is_bar else -grow) for k, n in enumerate(widths)]


def test_tables_agree_with_the_seven_module_codes():
    assert [tuple(_widths(s)) for s in dc.L_CODES] == do.L_WIDTHS
    assert [tuple(_widths(s)) for s in dc.R_CODES] == do.L_WIDTHS        # R: the same widths, a bar first
    assert [tuple(_widths(s)) for s in dc.G_CODES] == do.G_WIDTHS
    assert dc.PARITY == do.PARITY_WORDS
    assert dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])[-1] == 1 and dc.with_check([7, 3, 5, 1, 3, 5, 3])[-1] == 7   # published examples
    assert len(dc.runs(SYMBOLS[0])) == 59 and sum(dc.runs(SYMBOLS[0])) == 95
    assert len(dc.runs(SYMBOLS[3])) == 43 and sum(dc.runs(SYMBOLS[3])) == 67


@pytest.mark.parametrize("grow", [0, 200, -200])
def test_every_digit_of_every_set_decodes_to_itself(grow):
    """exact widths and +-20 % of a module of uniform bar growth"""
    for digit in range(10):
        assert do.decode_character(_grown(_widths(dc.L_CODES[digit]), False, grow), "LG") == ("L", digit)
        assert do.decode_character(_grown(_widths(dc.L_CODES[digit]), False, grow), "L") == ("L", digit)
        assert do.decode_character(_grown(_widths(dc.G_CODES[digit]), False, grow), "LG") == ("G", digit)
        assert do.decode_character(_grown(_widths(dc.R_CODES[digit]), True, grow), "R") == ("R", digit)


def test_the_pairs_that_share_their_edge_distances_are_told_apart():
    for a, b in ((1, 7), (2, 8)):
        for codes, sets, name, bar_first in ((dc.L_CODES, "LG", "L", False), (dc.G_CODES, "LG", "G", False), (dc.R_CODES, "R", "R", True)):
            wa, wb = _widths(codes[a]), _widths(codes[b])
            assert (wa[0] + wa[1], wa[1] + wa[2]) == (wb[0] + wb[1], wb[1] + wb[2])        # the same (E1, E2)
            for grow in (0, 150, -150):
                assert do.decode_character(_grown(wa, bar_first, grow), sets) == (name, a)
                assert do.decode_character(_grown(wb, bar_first, grow), sets) == (name, b)
    # halfway between the two patterns of a pair the distance to both is equal: a tie, rejected
    assert do.decode_character([2000, 2000, 2000, 1000], "L") == ("L", 1)
    assert do.decode_character([1000, 3000, 1000, 2000], "L") == ("L", 7)
    assert do.decode_character([1500, 2500, 1500, 1500], "L") is None


def _patch(frame, quad, pw, expand=1.25, ph=64):
    return opo.extract(frame[:, :, None], dc.int_quad(quad), ph, pw, None, expand)[0]


_RENDERS = {}


def _render(k, ppm, kind):
    key = (k, ppm, kind)
    if key not in _RENDERS:
        _RENDERS[key] = dc.render(SYMBOLS[k], ppm, ANGLES[k], seed=3 + k, **(dc.HARD if kind == "hard" else dc.CLEAN))
    return _RENDERS[key]


@pytest.mark.parametrize("kind", ["clean", "hard"])
@pytest.mark.parametrize("pw", [256, 384])
@pytest.mark.parametrize("ppm", [2, 3, 4])
def test_rendered_symbols_decode(ppm, pw, kind):
    for k, digits in enumerate(SYMBOLS):
        frame, quad = _render(k, ppm, kind)
        r = do.decode_patch(_patch(frame, quad, pw), min_votes=2)
        assert r[0] == len(digits) and r[3:3 + len(digits)] == digits and r[3 + len(digits):] == [-1] * (13 - len(digits)), (k, r)
        assert r[1] >= 2 and r[2] == 1, (k, r)


@pytest.mark.parametrize("kind", ["clean", "hard"])
@pytest.mark.parametrize("pw", [256, 384])
def test_no_wrong_payload_at_one_and_a_half_pixels_per_module(pw, kind):
    """a symbol may fail there; it may never be misread"""
    for k, digits in enumerate(SYMBOLS):
        frame, quad = _render(k, 1.5, kind)
        r = do.decode_patch(_patch(frame, quad, pw))
        assert r[0] == 0 or (r[0] == len(digits) and r[3:3 + len(digits)] == digits), (k, r)


def test_noise_and_random_stripes_give_none():
    rng = np.random.default_rng(17)
    none = [0, 0, 0] + [-1] * 13
    for _ in range(12):
        assert do.decode_patch(rng.integers(0, 256, (64, 256, 1), dtype=np.uint8)) == none
    for _ in range(12):
        row, x, v = np.zeros(256, np.uint8), 0, 0
        while x < 256:
            w = int(rng.integers(1, 9))
            row[x:x + w] = 225 if v else 35
            x, v = x + w, 1 - v
        assert do.decode_patch(np.broadcast_to(row[None, :, None], (64, 256, 1))) == none


def test_a_failing_checksum_gives_none():
    for digits in (SYMBOLS[0], SYMBOLS[3]):
        bad = list(digits)
        bad[-3] = (bad[-3] + 1) % 10
        assert do.decode_patch(dc.flat_patch([digits], 2, 64, 256, 20))[0] == len(digits)
        assert do.decode_patch(dc.flat_patch([bad], 2, 64, 256, 20)) == [0, 0, 0] + [-1] * 13


def test_a_cut_quiet_zone_gives_none():
    """a dark bar two modules before the symbol (QZ = 3) rejects it; four modules before it does not; the same behind it"""
    digits = SYMBOLS[0]
    for side in ("before", "behind"):
        for gap, want in ((2, 0), (4, 13)):
            patch = dc.flat_patch([digits], 2, 64, 256, 30).copy()
            x = 30 - 2 * gap - 6 if side == "before" else 30 + 2 * 95 + 2 * gap
            patch[:, x:x + 6] = 35
            r = do.decode_patch(patch)
            assert r[0] == want, (side, gap, r)
            if want:
                assert r[3:] == digits
    far = dc.flat_patch([digits], 2, 64, 256, 30).copy()
    far[:, 4:10] = 35                                                   # ten modules before the symbol
    assert do.decode_patch(far, quiet=8)[0] == 13 and do.decode_patch(far, quiet=16)[0] == 0
    assert do.decode_patch(dc.flat_patch([digits], 2, 64, 256, 30), quiet=16)[0] == 13     # no neighbouring edge: the border passes


def test_a_half_turned_patch_decodes_with_mask_two():
    for k in (0, 3):
        frame, quad = _render(k, 3, "clean")
        upright = _patch(frame, quad, 256)
        turned = _patch(frame, quad[4:] + quad[:4], 256)                 # the same object, the other long side on top
        assert np.array_equal(turned, upright[::-1, ::-1])
        a, b = do.decode_patch(upright), do.decode_patch(turned)
        assert a[2] == 1 and b[2] == 2 and a[:2] == b[:2] and a[3:] == b[3:] and a[0] == len(SYMBOLS[k])


def test_two_payloads_with_equal_votes_give_none():
    a, b = dc.flat_patch([SYMBOLS[0]], 2, 64, 256, 20), dc.flat_patch([SYMBOLS[2]], 2, 64, 256, 20)
    both = np.concatenate([a[:32], b[32:]])                             # lines 0..3 read one symbol, lines 4..7 the other
    assert do.decode_patch(both) == [0, 0, 0] + [-1] * 13
    more = np.concatenate([a[:40], b[40:]])                             # five lines against three
    r = do.decode_patch(more)
    assert r[:3] == [13, 5, 1] and r[3:] == SYMBOLS[0]
    assert do.decode_patch(more, min_votes=6)[0] == 0
    assert do.tally([(1, 13, (1,) * 13), (2, 13, (1,) * 13), (1, 8, (1,) * 8)], 2) == [13, 2, 3] + [1] * 13
    assert do.tally([(1, 13, (1,) * 13), (1, 8, (1,) * 8)], 1) == [0, 0, 0] + [-1] * 13


def test_the_lowest_start_counts_when_two_symbols_share_a_line():
    first, second = dc.with_check([5, 5, 1, 2, 3, 4, 5]), dc.with_check([9, 6, 3, 8, 5, 0, 7])
    patch = dc.flat_patch([first, second], 1, 8, 256, 40, gap=20)
    assert do.decode_patch(patch, scan_rows=1, min_votes=1) == [8, 1, 1] + first + [-1] * 5
    # the half-turned patch is read right to left, on the mirrored edge list, where the same symbol comes first again
    assert do.decode_patch(patch[::-1, ::-1], scan_rows=1, min_votes=1) == [8, 1, 2] + first + [-1] * 5
    e, l2d = do.line_edges(do.line_d(*do.line_profile(do.luma(patch), 0, 1, 1), 16, 24))
    assert do.line_votes(e, l2d, 256, 3, 3) == [(1, 8, tuple(first))]
    assert do.decode_candidate(e, l2d, 44, do.EAN8, 3) == second        # the second symbol is valid too: it starts 44 edges later


def _good_args():
    from ubdvss_amd import _lib
    params = _lib.UbdDecodeParams(3, 8, 1, 16, 24, 3, 2)
    fake = ctypes.c_void_p(0x1000)                                      # never dereferenced: every call below is refused before a launch
    return params, dict(patches=fake, counts=fake, n=2, cap=4, patch_h=64, patch_w=256, channels=3, params=ctypes.pointer(params),
                        results=fake, stream=None)


def test_every_refusal_of_the_entry_point():
    from ubdvss_amd import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES["ubd_decode_patches"][1]) == 10 and hasattr(lib, "ubd_decode_patches")
    _, good = _good_args()
    bad = [("patches", None, "patches"), ("counts", None, "counts"), ("params", None, "params"), ("results", None, "results"),
           ("n", 0, "n must"), ("n", -1, "n must"), ("cap", 0, "cap must"), ("cap", -2, "cap must"),
           ("patch_h", 0, "patch_h"), ("patch_h", 1025, "patch_h"), ("patch_w", 31, "patch_w"), ("patch_w", 1025, "patch_w"),
           ("channels", 0, "channels"), ("channels", 2, "channels"), ("channels", 4, "channels")]
    for name, value, word in bad:
        args = dict(good)
        args[name] = value
        assert lib.ubd_decode_patches(*args.values()) != 0, (name, value)
        msg = lib.ubd_last_error().decode()
        assert msg.startswith("ubd_decode_patches") and word in msg, (name, value, msg)
    fields = [("symbologies", (0, 4, -1)), ("scan_rows", (0, 33)), ("band", (-1, 9)), ("window", (0, 65)), ("contrast", (-1, 256)),
              ("quiet", (-1, 17)), ("min_votes", (0, 17))]
    for field, values in fields:
        for value in values:
            params, args = _good_args()
            setattr(params, field, value)
            assert lib.ubd_decode_patches(*args.values()) != 0, (field, value)
            msg = lib.ubd_last_error().decode()
            assert msg.startswith("ubd_decode_patches") and field in msg, (field, value, msg)
    params, args = _good_args()                                         # min_votes is bounded by 2 * scan_rows of the same call
    params.scan_rows, params.min_votes = 1, 3
    assert lib.ubd_decode_patches(*args.values()) != 0 and "min_votes" in lib.ubd_last_error().decode()
    _, args = _good_args()
    args.update(n=1 << 16, cap=1 << 15)
    assert lib.ubd_decode_patches(*args.values()) != 0 and "2^31" in lib.ubd_last_error().decode()


def test_python_seams():
    import torch
    import ubdvss_amd
    from ubdvss_amd import barcode_decoder as bd
    assert bd.DEFAULT_PARAMS == do.DEFAULTS
    p = bd.make_params(scan_rows=5, quiet=0)
    assert (p.symbologies, p.scan_rows, p.band, p.window, p.contrast, p.quiet, p.min_votes) == (3, 5, 1, 16, 24, 0, 2)
    with pytest.raises(TypeError):
        bd.make_params(rows=5)
    results = np.zeros((2, 3, 16), np.int32)
    results[0, 0] = [13, 6, 1] + SYMBOLS[1]
    results[0, 1] = [0, 0, 0] + [-1] * 13
    results[1, 0] = [8, 4, 2] + SYMBOLS[3] + [-1] * 5
    records = ubdvss_amd.results_to_records(results, np.array([2, 5], np.int32))
    assert [len(r) for r in records] == [2, 3]
    assert records[0][0] == ubdvss_amd.DecodedBarcode("EAN-13", "".join(map(str, SYMBOLS[1])), 6, False, True)
    assert records[0][1] is None and records[1][1] is None
    assert records[1][0] == ubdvss_amd.DecodedBarcode("EAN-8", "".join(map(str, SYMBOLS[3])), 4, True, False)
    if torch.cuda.is_available():
        return                                                          # the GPU tests run the rest
    with pytest.raises(RuntimeError):
        ubdvss_amd.decode_patches_on_device(np.zeros((1, 1, 8, 32, 1), np.uint8), np.zeros(1, np.int32))
    with pytest.raises(RuntimeError):
        ubdvss_amd.ModelRunner(ubdvss_amd.NetConfig(grey=False)).predict_decoded(None, [np.zeros((8, 8, 3), np.uint8)])
