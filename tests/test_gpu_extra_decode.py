"""GPU: UPC-E, Code 93 and Codabar in the three patch decoder kernels (ubd_decode_patches, ubd_decode_text_patches,
ubd_decode_width_patches) against the numpy restatement tests/extra_decode_oracle.py, which tests/test_extra_decode_host.py pins
on rendered symbols.  Every comparison is np.array_equal: no tolerance.  The result buffer is pre-filled with a sentinel and
carries guards at both ends: rows of slots without an object and the guards must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
from decode_cases import _noisy, _stripes, _tint  # noqa: E402
import extra_decode_cases as xc  # noqa: E402
import extra_decode_oracle as xo  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import width_decode_cases as wc  # noqa: E402
from test_extra_decode_host import (ACCEPTED, C93_TEXT, CBR_A, CBR_B, NONE16, NONE128, UPCE_A, UPCE_B, acceptance_patches, c93_row, cbr_row,  # noqa: E402,F401
                                    retail_row)
from ubdvss_amd import (_lib, NetConfig, Model, ModelRunner, DecodedBarcode, DecodedText, DecodedWidth, results_to_records,  # noqa: E402
                        text_results_to_records, width_results_to_records)

pytestmark = pytest.mark.gpu

GUARD = 64                                                              # elements of the result's type before and behind the rows
ENTRY = {"retail": "ubd_decode_patches", "text": "ubd_decode_text_patches", "width": "ubd_decode_width_patches"}
SENT = {"retail": -1515870811, "text": 0xA5, "width": 0xA5}
NONE = {"retail": NONE16, "text": NONE128, "width": NONE128}
EAN13_A, EAN8_A = dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3]), dc.with_check([5, 5, 1, 2, 3, 4, 5])
PARAM_SETS = [dict(scan_rows=1, band=0, window=1, contrast=0, min_votes=1), dict(scan_rows=32, band=8, window=64, contrast=255, min_votes=64),
              dict(scan_rows=8, band=8, window=1, contrast=255), dict(scan_rows=32, band=0, window=64, contrast=0, min_votes=1),
              dict(quiet=0), dict(quiet=16), dict(scan_rows=1, band=8, window=64, contrast=24, min_votes=2)]   # those of tests/test_gpu_decode.py

_LINES = {}                                                             # (patch bytes, shape, scan parameters) -> the edge lists of its scan lines


def _lines(patch, p):
    """the scan front end costs most of the oracle's time and does not depend on the symbologies: once per (patch, scan parameters)"""
    key = (patch.tobytes(), patch.shape, p["scan_rows"], p["band"], p["window"], p["contrast"])
    if key not in _LINES:
        _LINES[key] = xo.scan_lines(patch, p["scan_rows"], p["band"], p["window"], p["contrast"])
    return _LINES[key]


def _want(family, patches, counts, **kw):
    """xo.decode_patches(family, patches, counts, SENT, **kw) through the shared edge lists (test_the_shared_reference_is_the_oracle)"""
    p = dict(xo.DEFAULTS, **kw)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, xo.FAMILIES[family][3]), SENT[family], xo.FAMILIES[family][4])
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            out[i, j] = xo.decode_lines(family, _lines(patches[i, j], p), patches.shape[3], p["symbologies"], p["quiet"], p["min_votes"])
    return out


def _run_and_check(family, patches, counts, **kw):
    """one direct call of the family's C entry point; result rows, untouched rows and guards against the oracle.  Returns the rows."""
    lib = _lib.load()
    patches = np.ascontiguousarray(patches)
    n, cap, ph, pw, c = patches.shape
    row, dtype = xo.FAMILIES[family][3:]
    merged = dict(xo.DEFAULTS, **kw)
    params = _lib.UbdDecodeParams(*[merged[k] for k, _ in _lib.UbdDecodeParams._fields_])
    patches_d, counts_d = torch.from_numpy(patches).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    out = torch.full((2 * GUARD + n * cap * row,), SENT[family], dtype=torch.int32 if dtype == np.int32 else torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(lib, ENTRY[family])(patches_d.data_ptr(), counts_d.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params),
                                     out.data_ptr() + GUARD * out.element_size(), st)
    _lib.check(rc, ENTRY[family])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == SENT[family]).all() and (got[-GUARD:] == SENT[family]).all()
    got = got[GUARD:-GUARD].reshape(n, cap, row)
    want = _want(family, patches, counts, **kw)
    assert np.array_equal(got, want), [(i, j, got[i, j, :24].tolist(), want[i, j, :24].tolist())
                                       for i in range(n) for j in range(cap) if not np.array_equal(got[i, j], want[i, j])]
    return got


def _centred(mods, px, h=64, w=256, rng=None):
    g = xc.flat_patch([mods], px, h, w)[:, :, 0]
    return g if rng is None else _noisy(rng, g)


def _mixed(family, rng):
    """eight grey 64 x 256 patches of one family: new and old symbologies side by side, both directions, a symbol of each in one
    patch, stripes, noise and a flat patch"""
    if family == "retail":
        a, b, old = xc.upce_modules(UPCE_A), xc.upce_modules(UPCE_B), dc.modules(EAN13_A)
        both = xc.flat_patch([a, dc.modules(EAN8_A)], 1, 64, 256, gap=24)[:, :, 0]
        return [_centred(a, 3, rng=rng), _centred(b, 2, rng=rng)[::-1, ::-1], _centred(old, 2, rng=rng), both,
                _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8), np.full((64, 256), 200, np.uint8), _centred(dc.modules(EAN8_A), 2)[::-1, ::-1]]
    if family == "text":
        a, b, old = xc.c93_modules(xc.c93_values(C93_TEXT)), xc.c93_modules(xc.c93_values("aZ-9")), tc.modules(tc.encode_text("UBD1"))
        both = xc.flat_patch([xc.c93_modules(xc.c93_values("7")), tc.modules(tc.encode_text("12"))], 2, 64, 256, gap=24)[:, :, 0]
        return [_centred(a, 2, rng=rng), _centred(b, 3, rng=rng)[::-1, ::-1], _centred(old, 2, rng=rng), both,
                _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8), np.full((64, 256), 200, np.uint8), _centred(old, 2)[::-1, ::-1]]
    a, b = xc.cbr_modules(CBR_A, 2, 5), xc.cbr_modules(CBR_B, 2, 6)
    itf, c39 = wc.itf_modules("123456", 2, 5), wc.c39_modules("AB", 2, 5)
    both = xc.flat_patch([xc.cbr_modules("B7D", 2, 5), c39], 1, 64, 256, gap=16)[:, :, 0]
    return [_centred(a, 1, rng=rng), _centred(b, 1, rng=rng)[::-1, ::-1], _centred(itf, 1, rng=rng), both,
            _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8), np.full((64, 256), 200, np.uint8), _centred(c39, 1)[::-1, ::-1]]


@pytest.fixture(scope="module")
def mixed_patches():
    rng = np.random.default_rng(29)
    return {family: np.stack(_mixed(family, rng)).reshape(2, 4, 64, 256, 1) for family in ENTRY}


def test_the_shared_reference_is_the_oracle(mixed_patches):
    for family, patches in mixed_patches.items():
        for kw in (dict(symbologies=xo.FAMILIES[family][2]), dict(symbologies=ACCEPTED[ENTRY[family]][0], quiet=0, min_votes=1)):
            assert np.array_equal(_want(family, patches, [4, 3], **kw), xo.decode_patches(family, patches, [4, 3], SENT[family], **kw))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("family", list(ENTRY))
def test_mixed_patches_under_every_accepted_mask(mixed_patches, family, c):
    """counts [4, 3]: the last slot is not written.  Under the family's full mask every symbol is read, old and new, in its
    direction; the patch that holds one of each is a tie; under a single bit only that symbology's symbols are"""
    patches = _tint(mixed_patches[family][..., 0], c, seed=7)
    rows = {s: _run_and_check(family, patches, [4, 3], symbologies=s) for s in ACCEPTED[ENTRY[family]]}
    full, none = rows[xo.FAMILIES[family][2]], NONE[family]
    assert all((r[1, 3] == SENT[family]).all() for r in rows.values())
    new_a, new_b, old = {"retail": (retail_row(UPCE_A, 8, 1), retail_row(UPCE_B, 8, 2), [13, 8, 1] + EAN13_A),
                         "text": (c93_row(C93_TEXT, 8, 1), c93_row("aZ-9", 8, 2), None),
                         "width": (cbr_row(CBR_A, 8, 1), cbr_row(CBR_B, 8, 2), None)}[family]
    assert full[0, 0].tolist() == new_a and full[0, 1].tolist() == new_b and full[0, 2, 0] in (13, 128, 25) and full[0, 3].tolist() == none
    assert [full[1, j].tolist() for j in range(3)] == [none] * 3
    if old is not None:
        assert full[0, 2].tolist() == old
    new_bit = {"retail": 64, "text": 128, "width": 256}[family]
    assert rows[new_bit][0, 0].tolist() == new_a and rows[new_bit][0, 2].tolist() == none and rows[new_bit][0, 3, 0] in (6, 93, 27)
    for s, r in rows.items():
        if not s & new_bit:                                             # an older mask: nothing of the new symbologies, and the older rows as under the full mask
            assert r[0, 0].tolist() == none and r[0, 1].tolist() == none
            if s == xo.FAMILIES[family][2] & ~new_bit:
                assert np.array_equal(r[0, 2], full[0, 2])


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
@pytest.mark.parametrize("family", list(ENTRY))
def test_parameter_extremes(mixed_patches, family, kw):
    new_bit = {"retail": 64, "text": 128, "width": 256}[family]
    for symbologies in (new_bit, xo.FAMILIES[family][2]):
        _run_and_check(family, mixed_patches[family], [4, 4], symbologies=symbologies, **kw)


@pytest.mark.parametrize("group", ["retail", "text", "width-2", "width-3"])
def test_the_acceptance_set(acceptance_patches, group):  # noqa: F811
    """the 216 patches of tests/test_extra_decode_host.py (64 x 256 and 64 x 384, 16 a call), grey and tinted in turn, under the
    symbology's own bit: the device reads each as the oracle does, which is as it was drawn"""
    family = group.split("-")[0]
    mine = [(row, mask, patch) for fam, _, row, mask, patch in acceptance_patches if fam == family]
    if family == "width":
        half = len(mine) // 2
        mine = mine[:half] if group == "width-2" else mine[half:]
    bit = {"retail": 64, "text": 128, "width": 256}[family]
    for pw in (256, 384):
        sized = [m for m in mine if m[2].shape[1] == pw]
        for k0 in range(0, len(sized), 16):
            part = sized[k0:k0 + 16]
            if len(part) % 4:
                part = part + [part[-1]] * (4 - len(part) % 4)
            grey = np.stack([m[2][:, :, 0] for m in part]).reshape(len(part) // 4, 4, 64, pw)
            got = _run_and_check(family, _tint(grey, 1 + 2 * ((k0 // 16) % 2), seed=k0), [4] * (len(part) // 4), symbologies=bit)
            for k, (row, mask, _) in enumerate(part):
                r = got[k // 4, k % 4].tolist()
                assert r[1] >= 2 and r == row(r[1], mask), (group, pw, k0 + k, r[:12])


def test_an_ean13_whose_left_half_is_a_upce_reads_as_ean13():
    """first digit 1, the left half a valid UPC-E of number system 1 (checked on the CPU: without the five-module rule the oracle's
    UPC-E reader accepts it): EAN-13 under 67, nothing under 64"""
    left = next(six for six in ([int(ch) for ch in f"{v:06d}"] for v in range(1000000)) if xo.upca_check([1] + xo.upce_expand(six)) == 1)
    ean = dc.with_check([1] + left + [3, 0, 0, 0, 0])
    patch = dc.flat_patch([ean], 2, 64, 256, 30)
    e, l2d = xo.scan_lines(patch, 1, 0, 16, 24)[0]
    assert xo.upce_candidate(e, l2d, 0, 3, trailing=0) == [1] + left + [1] and xo.upce_candidate(e, l2d, 0, 3) is None
    patches = np.stack([patch, patch[::-1, ::-1]]).reshape(1, 2, 64, 256, 1)
    got = _run_and_check("retail", patches, [2], symbologies=67)
    assert got[0, 0].tolist() == [13, 8, 1] + ean and got[0, 1].tolist() == [13, 8, 2] + ean
    for quiet in (0, 3):
        got = _run_and_check("retail", patches, [2], symbologies=64, quiet=quiet, min_votes=1)
        assert got[0, 0].tolist() == NONE16 and got[0, 1].tolist() == NONE16


def test_lengths_every_character_and_wide_patches():
    """13 x 1024: all 47 values of Code 93 and sixty data characters, sixty-one are one too many; all twenty Codabar characters,
    sixty data characters and sixty-one; every UPC-E digit in both sets"""
    rng = np.random.default_rng(3)
    long = "".join(xc.C93_ALPHABET[int(v)] for v in rng.integers(0, 47, 61))
    texts = [xc.C93_ALPHABET, long[:60], long, xc.C93_ALPHABET[::-1]]
    grey = [xc.flat_patch([xc.c93_modules(xc.c93_values(t))], 1, 13, 1024)[:, :, 0] for t in texts]
    got = _run_and_check("text", np.stack(grey).reshape(1, 4, 13, 1024, 1), [4], symbologies=132)
    assert [got[0, j].tolist() for j in range(4)] == [c93_row(texts[0], 8, 1), c93_row(texts[1], 8, 1), NONE128, c93_row(texts[3], 8, 1)]
    data = "".join(xo.CBR_CHARS[int(v)] for v in rng.integers(0, 16, 61))
    texts = ["A" + xo.CBR_CHARS[:16] + "B", "C" + data[:60] + "D", "C" + data + "D", "D" + xo.CBR_CHARS[15::-1] + "C"]
    grey = [xc.flat_patch([xc.cbr_modules(t, 1, 2)], 1, 13, 1024)[:, :, 0] for t in texts]
    grey[3] = grey[3][::-1, ::-1]
    got = _run_and_check("width", np.stack(grey).reshape(1, 4, 13, 1024, 1), [4], symbologies=280)
    assert [got[0, j].tolist() for j in range(4)] == [cbr_row(texts[0], 8, 1), cbr_row(texts[1], 8, 1), NONE128, cbr_row(texts[3], 8, 2)]
    eights = [xc.upce_digits(0, "012345"), xc.upce_digits(1, "678901"), xc.upce_digits(0, "987654"), xc.upce_digits(1, "321098")]
    grey = [xc.flat_patch([xc.upce_modules(d)], 1 + 2 * (k % 2), 13, 1024)[:, :, 0] for k, d in enumerate(eights)]
    got = _run_and_check("retail", np.stack(grey).reshape(1, 4, 13, 1024, 1), [4], symbologies=67)
    assert [got[0, j].tolist() for j in range(4)] == [retail_row(d, 8, 1) for d in eights]
    stripes = np.broadcast_to(np.where(np.arange(1024) % 2, 225, 35).astype(np.uint8)[None, :], (13, 1024))     # 1023 edges
    for family in ENTRY:
        got = _run_and_check(family, np.stack([stripes, stripes[:, ::-1]]).reshape(1, 2, 13, 1024, 1), [2], symbologies=xo.FAMILIES[family][2], quiet=0, min_votes=1)
        assert got[0, 0].tolist() == NONE[family] and got[0, 1].tolist() == NONE[family]


def test_small_and_odd_patch_sizes():
    """1 x 32 holds no symbol and runs all the same; 5 x 95 holds a UPC-E, a short Code 93 and a short Codabar at one pixel per module"""
    rng = np.random.default_rng(5)
    for family, mods, row in (("retail", xc.upce_modules(UPCE_A), retail_row(UPCE_A, 8, 1)), ("text", xc.c93_modules(xc.c93_values("7")), c93_row("7", 8, 1)),
                              ("width", xc.cbr_modules("A1B", 1, 3), cbr_row("A1B", 8, 1))):
        tiny = rng.integers(0, 256, (2, 2, 1, 32, 3), dtype=np.uint8)
        assert (_run_and_check(family, tiny, [1, 0], symbologies=xo.FAMILIES[family][2])[1] == SENT[family]).all()
        g = xc.flat_patch([mods], 1, 5, 95)[:, :, 0]
        grey = np.stack([g, g[::-1, ::-1], _stripes(rng, 5, 95), g]).reshape(2, 2, 5, 95)
        got = _run_and_check(family, _tint(grey, 3, seed=3), [2, 1], symbologies=xo.FAMILIES[family][2])
        assert got[0, 0].tolist() == row and got[0, 1, :3].tolist() == [row[0], 8, 2] and got[1, 0].tolist() == NONE[family]
        assert (got[1, 1] == SENT[family]).all()


def test_refusals_leave_the_results_untouched(mixed_patches):
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for family, entry in ENTRY.items():
        patches_d, counts_d = torch.from_numpy(mixed_patches[family]).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
        out = torch.full((2 * 4 * 128,), 0xA5, dtype=torch.uint8, device="cuda")
        for value in (0, 32, 63, 479, 511, 512, -1) + tuple(v for e, vs in ACCEPTED.items() if e != entry for v in vs):
            params = _lib.UbdDecodeParams(value, 8, 1, 16, 24, 3, 2)
            assert getattr(lib, entry)(patches_d.data_ptr(), counts_d.data_ptr(), 2, 4, 64, 256, 1, ctypes.byref(params), out.data_ptr(), st) != 0, (entry, value)
            assert lib.ubd_last_error().decode().startswith(entry) and "symbologies" in lib.ubd_last_error().decode()
        torch.cuda.synchronize()
        assert (out == 0xA5).all()


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


def test_predict_decoded_reads_all_eight_kinds(golden_dir):
    """The golden detection weights are a random initialisation: at pixel_threshold 0.3 every pixel is positive and each frame
    yields one box, its whole frame (tests/test_gpu_object_patches.py).  The frames are upright symbols with quiet zones, one of
    every kind the three kernels read."""
    from oracle import net_numpy as onet
    d = np.load(os.path.join(golden_dir, "net_rgb_det.npz"))
    cfg = NetConfig(grey=False, fml_compatible=bool(d["fml"]))
    model = Model(cfg)
    model.set_weights(onet.unflatten_weights(d["params"], 3, 0))
    runner = ModelRunner(cfg, pixel_threshold=0.3, max_objects_per_image=16)
    itf, c39, cbr = wc.itf_modules("123456", 3, 8), wc.c39_modules("AB", 3, 8), xc.cbr_modules("A12B", 3, 8)
    frames = [dc.flat_patch([EAN13_A], 3, 120, 320, 17, channels=3), dc.flat_patch([EAN8_A], 3, 120, 320, 60, channels=3),
              xc.flat_patch([xc.upce_modules(UPCE_A)], 3, 120, 320, channels=3), tc.flat_patch([tc.encode_text("UBD1")], 3, 120, 320, 40, channels=3),
              xc.flat_patch([xc.c93_modules(xc.c93_values("UBD"))], 3, 120, 320, channels=3), xc.flat_patch([itf], 1, 120, 320, channels=3),
              xc.flat_patch([c39], 1, 120, 320, channels=3), xc.flat_patch([cbr], 1, 120, 320, channels=3)]
    found, decoded = runner.predict_decoded(model, frames, symbologies=479)
    assert [_key(o) for o in found] == [_key(o) for o in runner.predict_images(model, frames)]
    assert [len(o) for o in found] == [1] * 8 and [len(r) for r in decoded] == [1] * 8
    records = [r[0] for r in decoded]
    assert [type(r) for r in records] == [DecodedBarcode] * 3 + [DecodedText] * 2 + [DecodedWidth] * 3
    assert [r.symbology for r in records] == ["EAN-13", "EAN-8", "UPC-E", "Code 128", "Code 93", "ITF", "Code 39", "Codabar"]
    assert [r.text for r in records] == ["".join(map(str, EAN13_A)), "".join(map(str, EAN8_A)), "01234565", "UBD1", "UBD", "123456", "AB", "A12B"]
    assert not records[2].is_upc_a and not records[4].gs1 and all(r.votes >= 2 for r in records)
    # the records are the oracle's readings of the very patches predict_patches returns
    _, patches = runner.predict_patches(model, frames, expand=1.25)
    for k in range(8):
        family, to_records = (("retail", results_to_records), ("text", text_results_to_records), ("width", width_results_to_records))[(k >= 3) + (k >= 5)]
        want = xo.decode_patches(family, patches[k][None], [1], 0, symbologies=479 & xo.FAMILIES[family][2])
        assert decoded[k] == to_records(want, [1])[0], k
    assert [r[0] for r in runner.predict_decoded(model, frames, symbologies=64 | 128 | 256)[1]] == [None, None, records[2], None, records[4], None, None, records[7]]
    assert [r[0] for r in runner.predict_decoded(model, frames, symbologies=31)[1]] == records[:2] + [None, records[3], None] + records[5:7] + [None]
    for value in (32, 63, 511, 512, -1):
        with pytest.raises(ValueError):
            runner.predict_decoded(model, frames, symbologies=value)
