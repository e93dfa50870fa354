"""GPU: ubd_decode_text_patches (Code 128 / GS1-128 out of the object patches) against the numpy restatement
tests/text_decode_oracle.py, which tests/test_text_decode_host.py pins on rendered symbols.  Every comparison is np.array_equal:
no tolerance.  The result buffer is pre-filled with a sentinel and carries guard bytes at both ends: rows of slots without an
object and the guards must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
from decode_cases import _noisy, _row_from_pixel_runs, _stripes, _tint  # noqa: E402
import decode_oracle as do  # noqa: E402
import object_patches_oracle as opo  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import text_decode_oracle as to  # noqa: E402
from ubdvss_amd import (_lib, NetConfig, Model, ModelRunner, DecodedBarcode, DecodedText, decode_text_patches_on_device,  # noqa: E402
                        extract_objects_on_device, results_to_records, text_results_to_records)

pytestmark = pytest.mark.gpu

SENT, GUARD, ROW = 0xA5, 64, 128
NONE = [0] * 8 + [0xFF] * 120
A, B, C = tc.START_A, tc.START_B, tc.START_C
SHORT_A, SHORT_B, GS1 = tc.encode_text("AB12"), tc.encode_text("x-9Z"), tc.encode_text("0112", True)
TEXT_A, TEXT_B = tc.encode_text("UBD-4711/AMD"), tc.encode_text("a\tB\x00c 20261020 Zz")
EAN13_A = dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])


def _params(**kw):
    merged = dict(to.DEFAULTS, **kw)
    return _lib.UbdDecodeParams(*[merged[k] for k, _ in _lib.UbdDecodeParams._fields_])


def _call(lib, patches_d, counts_d, shape, params, out):
    n, cap, ph, pw, c = shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.ubd_decode_text_patches(patches_d.data_ptr(), counts_d.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params),
                                       out.data_ptr() + GUARD, st)


def _row(values, votes, mask):
    """the result row of a symbol read with ``votes`` votes, from the encoder's values and the oracle's text rule"""
    text = to.text_elements(values)
    return [128, votes, mask, len(text), int(values[1] == 102), len(values) - 2, values[0], values[-1]] + text + [0xFF] * (120 - len(text))


def _run_and_check(patches, counts, **kw):
    """one direct call of the C entry point; result rows, untouched rows and guards against the oracle.  Returns the rows."""
    lib = _lib.load()
    patches = np.ascontiguousarray(patches)
    n, cap = patches.shape[:2]
    patches_d, counts_d = torch.from_numpy(patches).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    out = torch.full((2 * GUARD + n * cap * ROW,), SENT, dtype=torch.uint8, device="cuda")
    _lib.check(_call(lib, patches_d, counts_d, patches.shape, _params(**kw), out), "ubd_decode_text_patches")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
    got = got[GUARD:-GUARD].reshape(n, cap, ROW)
    want = to.decode_patches(patches, counts, SENT, **kw)
    assert np.array_equal(got, want), [(i, j, got[i, j, :24].tolist(), want[i, j, :24].tolist())
                                       for i in range(n) for j in range(cap) if not np.array_equal(got[i, j], want[i, j])]
    return got


def _symbol(h, w, values, rng=None):
    """the widest upright drawing of the symbol that leaves five modules of quiet zone in w pixels (None: it does not fit)"""
    m = len(tc.modules(values))
    px = w // (m + 10)
    if px < 1:
        return None
    g = tc.flat_patch([values], px, h, w, (w - m * px) // 2)[:, :, 0]
    return g if rng is None else _noisy(rng, g)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("ph,pw", [(1, 32), (5, 95), (64, 256), (13, 1024)])
def test_patch_sizes_channels_and_counts(ph, pw, c):
    """n = 3, cap = 2, counts [0, 2, cap + 1]: image 0 holds valid symbols that must not be read; at width 32 no symbol fits
    (start, one character, check and stop are 46 modules) and the call runs all the same; 95 holds 89 modules at one pixel each"""
    rng = np.random.default_rng(ph * 1000 + pw)
    kinds = [_symbol(ph, pw, SHORT_A, rng), _symbol(ph, pw, GS1, rng), _symbol(ph, pw, SHORT_B), _symbol(ph, pw, SHORT_A)]
    kinds = [k for k in kinds if k is not None] + [_stripes(rng, ph, pw), _stripes(rng, ph, pw, 1, 3), rng.integers(0, 256, (ph, pw), dtype=np.uint8)]
    grey = np.stack([kinds[0], kinds[1], kinds[0], kinds[1][::-1, ::-1], kinds[2], kinds[-1]]).reshape(3, 2, ph, pw)
    got = _run_and_check(_tint(grey, c, seed=pw), [0, 2, 3])
    assert (got[0] == SENT).all()
    if pw == 256:                                                       # (at 1024 a run is wider than the default window)
        assert got[1, 0].tolist() == _row(SHORT_A, 8, 1) and got[1, 1].tolist() == _row(GS1, 8, 2)     # upright; half-turned


# the seven parameter-extreme sets of tests/test_gpu_decode.py, with the one symbology of this entry point
PARAM_SETS = [dict(scan_rows=1, band=0, window=1, contrast=0, min_votes=1), dict(scan_rows=32, band=8, window=64, contrast=255, min_votes=64),
              dict(scan_rows=8, band=8, window=1, contrast=255), dict(scan_rows=32, band=0, window=64, contrast=0, min_votes=1),
              dict(symbologies=4, quiet=0), dict(symbologies=4, quiet=16), dict(scan_rows=1, band=8, window=64, contrast=24, min_votes=2)]


@pytest.fixture(scope="module")
def mixed_patches():
    """64 x 256 x 1: noisy symbols in both directions, stripes, noise, a faint symbol (contrast clamp), two payloads"""
    rng = np.random.default_rng(23)
    faint = (128 + (tc.flat_patch([SHORT_A], 2, 64, 256, 33)[:, :, 0].astype(np.int32) - 128) // 16).astype(np.uint8)
    two = np.concatenate([_symbol(64, 256, SHORT_A)[:32], _symbol(64, 256, SHORT_B)[32:]])
    grey = [_symbol(64, 256, SHORT_A, rng), _symbol(64, 256, GS1, rng)[::-1, ::-1], _symbol(64, 256, SHORT_B, rng)[::-1, ::-1],
            _symbol(64, 256, GS1, rng), _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8), faint, two]
    return np.stack(grey).reshape(2, 4, 64, 256, 1)


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_parameter_extremes(mixed_patches, kw):
    got = _run_and_check(mixed_patches, [4, 4], **kw)
    if kw == dict(symbologies=4, quiet=0):
        assert got[0, 0].tolist() == _row(SHORT_A, 8, 1) and got[0, 1].tolist() == _row(GS1, 8, 2) and got[1, 3].tolist() == NONE


def test_defaults_on_the_mixed_patches(mixed_patches):
    got = _run_and_check(mixed_patches, [4, 4])
    assert [got[0, j].tolist() for j in range(4)] == [_row(SHORT_A, 8, 1), _row(GS1, 8, 2), _row(SHORT_B, 8, 2), _row(GS1, 8, 1)]
    assert [got[1, j].tolist() for j in range(4)] == [NONE] * 4          # stripes, noise, below the contrast, a tie of two payloads
    assert _run_and_check(mixed_patches, [4, 4], contrast=2)[1, 2].tolist() == _row(SHORT_A, 8, 1)     # the faint one, once allowed


def _walk(values):
    """(set a data value is read in, value) for every data value, by the switches alone: the test's own bookkeeping of which
    table cells the symbols below reach"""
    cur, shift, out = "ABC"[values[0] - A], False, []
    for v in values[1:-1]:
        code = cur if cur == "C" or not shift else "AB"[cur == "A"]
        shift = False
        out.append((code, v))
        if code == "C":
            cur = {100: "B", 101: "A"}.get(v, cur)
        elif v == 98:
            shift = True
        elif v == 99:
            cur = "C"
        elif (code, v) in (("A", 100), ("B", 101)):
            cur = "B" if code == "A" else "A"
    return out


def coverage_symbols():
    r = lambda a, b: list(range(a, b))  # noqa: E731
    data = [(A, r(0, 60)),
            (A, r(60, 98) + [102, 101, 98, 65, 100] + r(0, 16)),                    # FNC1, FNC4, Shift + 'a' (set B), Code B
            (B, r(16, 76)),
            (B, r(76, 98) + [102, 100, 98, 65, 101, 99] + r(0, 30)),                # FNC1, FNC4, Shift + SOH (set A), Code A, Code C
            (C, r(30, 90)),
            (C, r(90, 100) + [102, 100, 99, 101, 98])]                              # FNC1, Code B, Code C, Code A, a trailing Shift
    return [tc.values_with_check(s, d) for s, d in data] + [tc.encode_text("0112345678901231" + tc.FNC1 + "10AB", True), TEXT_B]


def test_every_value_of_every_set_in_one_call():
    """eight symbols at one pixel per module, upright and half-turned in turn: every value 0..102 as data in sets A, B and C (in
    C: every pair 00..99, both switches and FNC1), all three starts, Shift in both directions and as the last data character,
    FNC1 first (the flag) and later, control characters"""
    symbols = coverage_symbols()
    seen = {cell for s in symbols for cell in _walk(s)}
    assert seen == {(code, v) for code in "ABC" for v in range(103)}
    assert {s[0] for s in symbols} == {A, B, C} and symbols[5][-2] == 98 and symbols[6][1] == 102 and 102 in symbols[6][2:-1]
    assert ("B", 98) in _walk(symbols[3])[:-1] and ("A", 98) in _walk(symbols[1])[:-1]      # a Shift in B (to A) and in A (to B)
    assert any(v < 32 for v in to.text_elements(TEXT_B)) and 1 in to.text_elements(symbols[3])
    grey = np.stack([_symbol(8, 1024, s) if k % 2 else _symbol(8, 1024, s)[::-1, ::-1] for k, s in enumerate(symbols)])
    got = _run_and_check(grey.reshape(2, 4, 8, 1024, 1), [4, 4], scan_rows=2, band=0)
    for k, s in enumerate(symbols):
        assert got[k // 4, k % 4].tolist() == _row(s, 2, 1 if k % 2 else 2), k
    assert got[1, 2, 4] == 1 and [int(got[k // 4, k % 4, 4]) for k in range(6)] == [0] * 6     # the GS1 flag
    assert got[1, 1, 3] == 2 * 10 + 1 and got[1, 0, 3] == 120                                 # the trailing Shift left no element; T at its bound


def test_the_length_limit_and_the_most_edges_a_line_can_hold():
    """60 data characters at one pixel per module (706 modules) are read, 61 are one value too many; 1024 pixels of alternating
    1-pixel stripes are 1023 edges, every other one a candidate start, both ways"""
    rng = np.random.default_rng(3)
    sixty, sixty_one = tc.values_with_check(B, rng.integers(0, 96, 60)), tc.values_with_check(B, rng.integers(0, 96, 61))
    stripes = np.broadcast_to(np.where(np.arange(1024) % 2, 225, 35).astype(np.uint8)[None, :], (13, 1024))
    e, _ = do.line_edges(do.line_d(*do.line_profile(do.luma(stripes), 0, 8, 1), 16, 24))
    assert len(e) == 1023
    patches = np.stack([_symbol(13, 1024, sixty), _symbol(13, 1024, sixty_one), stripes, stripes[:, ::-1]]).reshape(1, 4, 13, 1024, 1)
    got = _run_and_check(patches, [4])
    assert got[0, 0].tolist() == _row(sixty, 8, 1) and [got[0, j].tolist() for j in (1, 2, 3)] == [NONE] * 3
    _run_and_check(patches, [4], scan_rows=32, band=8, window=64, quiet=0, min_votes=1)


def test_two_symbols_side_by_side_the_lowest_start_counts():
    patch = tc.flat_patch([SHORT_A, SHORT_B], 1, 8, 256, 30, gap=20)
    patches = np.stack([patch, patch[::-1, ::-1]]).reshape(1, 2, 8, 256, 1)
    got = _run_and_check(patches, [2], scan_rows=1, min_votes=1)
    assert got[0, 0].tolist() == _row(SHORT_A, 1, 1) and got[0, 1].tolist() == _row(SHORT_A, 1, 2)
    got = _run_and_check(patches, [2], scan_rows=5, band=0)
    assert got[0, 0, :3].tolist() == [128, 5, 1]


def test_rejections_check_value_bar_sum_and_tie():
    """a wrong check value; a character whose bars are redrawn 0.6 module thinner and its spaces as much wider, which keeps
    every edge-to-similar-edge distance and moves the bar sum by 1.8 modules of the 1.5 allowed; two payloads with four lines each"""
    bad = SHORT_A[:-1] + [(SHORT_A[-1] + 1) % 103]
    runs_px = [5 * r for r in tc.runs(SHORT_A)]
    exact = np.broadcast_to(_row_from_pixel_runs(runs_px, 512, 40)[None, :], (64, 512))
    runs_px[12:18] = [w + (-3 if k % 2 == 0 else 3) for k, w in enumerate(runs_px[12:18])]     # the second data character
    redrawn = np.broadcast_to(_row_from_pixel_runs(runs_px, 512, 40)[None, :], (64, 512))
    e, _ = do.line_edges(do.line_d(*do.line_profile(do.luma(redrawn), 0, 8, 1), 16, 24))
    w6 = [e[13 + k] - e[12 + k] for k in range(6)]
    assert to.decode_character(w6) is None                              # the rejection itself, and that it is the bar-sum test's
    assert tuple((22 * (w6[k] + w6[k + 1]) + sum(w6)) // (2 * sum(w6)) for k in range(4)) in to.KEYS
    assert to.decode_patch(redrawn[:, :, None], min_votes=1) == NONE and to.decode_patch(exact[:, :, None]) == _row(SHORT_A, 8, 1)
    tie = np.concatenate([_symbol(64, 512, SHORT_A)[:32], _symbol(64, 512, SHORT_B)[32:]])
    patches = np.stack([_symbol(64, 512, bad), redrawn, tie, exact]).reshape(1, 4, 64, 512, 1)
    got = _run_and_check(patches, [4])
    assert [got[0, j].tolist() for j in range(4)] == [NONE] * 3 + [_row(SHORT_A, 8, 1)]
    got = _run_and_check(patches, [4], min_votes=1, quiet=0)
    assert [got[0, j].tolist() for j in range(3)] == [NONE] * 3


@pytest.fixture(scope="module")
def rendered():
    """frames with a Code 128 and a GS1-128 at 3 and 2 pixels per module, blurred, noisy and unevenly lit, and their true quads"""
    gs1 = tc.encode_text("0109501101530003171407041012345", True)
    return [(TEXT_A, ) + tc.render(TEXT_A, 3, -33.0, seed=5, **dc.HARD), (gs1, ) + tc.render(gs1, 2, 101.0, seed=6, **dc.HARD)]


def test_rendered_symbols_in_both_directions(rendered):
    grey = []
    for _, frame, quad in rendered:
        q = dc.int_quad(quad)
        grey += [opo.extract(frame[:, :, None], q, 64, 512, None, 1.25)[0][:, :, 0], opo.extract(frame[:, :, None], q[4:] + q[:4], 64, 512, None, 1.25)[0][:, :, 0]]
    for c in (1, 3):
        got = _run_and_check(_tint(np.stack(grey).reshape(2, 2, 64, 512), c, seed=9), [2, 2])
        for i, (values, _, _) in enumerate(rendered):
            for j in range(2):
                assert got[i, j, 1] >= 2 and got[i, j].tolist() == _row(values, int(got[i, j, 1]), 1 + j), (c, i, j, got[i, j, :8])


def test_graph_capture_equals_the_direct_call(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    params = _params()
    nbytes = 2 * GUARD + 2 * 4 * ROW
    direct = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")

    def call(o):
        _lib.check(_call(lib, patches_d, counts_d, mixed_patches.shape, params, o), "ubd_decode_text_patches")
    call(direct)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(out)                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # captures on a side stream of its own
        call(out)
    out.fill_(SENT)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, direct)
    rows = direct[GUARD:-GUARD].cpu().numpy().reshape(2, 4, ROW)
    assert rows[0, 0, 0] == 128 and (rows[1, 3] == SENT).all()


def test_refusals_leave_the_results_untouched(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + 2 * 4 * ROW,), SENT, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for field, value in (("symbologies", 0), ("symbologies", 3), ("symbologies", 7), ("scan_rows", 0), ("scan_rows", 33), ("band", -1), ("band", 9),
                         ("window", 0), ("window", 65), ("contrast", -1), ("contrast", 256), ("quiet", -1), ("quiet", 17), ("min_votes", 0),
                         ("min_votes", 17)):
        p = _params(**{field: value})
        assert _call(lib, patches_d, counts_d, mixed_patches.shape, p, out) != 0, (field, value)
        assert lib.ubd_last_error().decode().startswith("ubd_decode_text_patches")
    for shape in ((2, 4, 64, 31, 1), (2, 4, 64, 1025, 1), (2, 4, 1025, 256, 1), (2, 4, 0, 256, 1), (2, 4, 64, 256, 2), (0, 4, 64, 256, 1), (2, 0, 64, 256, 1)):
        assert _call(lib, patches_d, counts_d, shape, _params(), out) != 0
    good = [patches_d.data_ptr(), counts_d.data_ptr(), 2, 4, 64, 256, 1, ctypes.byref(_params()), out.data_ptr() + GUARD, st]
    for k in (0, 1, 7, 8):                                              # a null pointer in each pointer's place
        assert lib.ubd_decode_text_patches(*[None if q == k else a for q, a in enumerate(good)]) != 0
    assert lib.ubd_decode_text_patches(*good[:8], out.data_ptr() + GUARD + 1, st) != 0        # rows leave as dwords
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert _call(lib, patches_d, counts_d, mixed_patches.shape, _params(), out) == 0     # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert (out[GUARD:-GUARD] != SENT).any() and (out[:GUARD] == SENT).all() and (out[-GUARD:] == SENT).all()


def test_python_seam_extract_then_decode(rendered):
    """extract_objects_on_device on the rendered frames with their true quads, then decode_text_patches_on_device: the encoded text"""
    frames = [np.repeat(f[:, :, None], 3, axis=2) for _, f, _ in rendered]
    quads = np.zeros((2, 2, 8), np.int32)
    quads[0, 0], quads[1, 0] = dc.int_quad(rendered[0][2]), dc.int_quad(rendered[1][2])
    quads[1, 1] = quads[1, 0][[4, 5, 6, 7, 0, 1, 2, 3]]
    counts = np.array([1, 2], np.int32)
    patches = extract_objects_on_device(frames, quads, counts, patch_size=(64, 512), expand=1.25)
    results = decode_text_patches_on_device(patches, counts)
    assert results.shape == (2, 2, 128) and results.dtype == torch.uint8 and results.is_cuda
    want = to.decode_patches(patches.cpu().numpy(), counts, 0)
    want[0, 1, 8:] = 0xFF                                               # the empty slot reads as "none"
    assert np.array_equal(results.cpu().numpy(), want)
    records = text_results_to_records(results, counts)
    assert [len(r) for r in records] == [1, 2]
    plain, gs1 = records[0][0], records[1][0]
    assert plain == DecodedText("Code 128", "UBD-4711/AMD", plain.votes, False, False, tuple(b"UBD-4711/AMD")) and plain.votes >= 2
    assert gs1.text == "0109501101530003171407041012345" and gs1.gs1 and not gs1.upside_down and gs1.elements[0] == 0xF1
    assert gs1.elements[1:] == tuple(gs1.text.encode()) and records[1][1] == gs1._replace(upside_down=True, votes=records[1][1].votes)
    more = text_results_to_records(decode_text_patches_on_device(patches, torch.from_numpy(counts).cuda(), scan_rows=16, symbologies=4), counts)
    assert more[0][0].text == plain.text and more[1][1].upside_down
    with pytest.raises(TypeError):
        decode_text_patches_on_device(patches, counts, rows=4)
    with pytest.raises(RuntimeError, match="ubd_decode_text_patches"):
        decode_text_patches_on_device(patches, counts, symbologies=3)


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


def test_predict_decoded_with_the_golden_detection_weights(golden_dir):
    """The golden detection weights are a random initialisation: at pixel_threshold 0.3 every pixel is positive and each frame
    yields one box, its whole frame (tests/test_gpu_object_patches.py).  The frames are upright symbols with quiet zones: a
    Code 128, a GS1-128 and an EAN-13."""
    from oracle import net_numpy as onet
    d = np.load(os.path.join(golden_dir, "net_rgb_det.npz"))
    cfg = NetConfig(grey=False, fml_compatible=bool(d["fml"]))
    model = Model(cfg)
    model.set_weights(onet.unflatten_weights(d["params"], 3, 0))
    runner = ModelRunner(cfg, pixel_threshold=0.3, max_objects_per_image=16)
    code128, gs1 = tc.encode_text("UBD1"), tc.encode_text("0112", True)
    frames = [tc.flat_patch([code128], 3, 120, 320, 40, channels=3), tc.flat_patch([gs1], 3, 120, 320, 58, channels=3),
              dc.flat_patch([EAN13_A], 3, 120, 320, 17, channels=3)]
    want_found = runner.predict_images(model, frames)
    found, decoded = runner.predict_decoded(model, frames, symbologies=7)
    assert [_key(o) for o in found] == [_key(o) for o in want_found]
    assert [len(o) for o in found] == [1, 1, 1] and [len(r) for r in decoded] == [1, 1, 1]
    a, b, c = (r[0] for r in decoded)
    # (which long side of the whole-frame box lands on top is the extraction's choice: upside_down is the oracle's to say, below)
    assert isinstance(a, DecodedText) and (a.text, a.gs1, a.elements) == ("UBD1", False, tuple(b"UBD1")) and a.votes >= 2
    assert isinstance(b, DecodedText) and (b.text, b.gs1, b.elements) == ("0112", True, (0xF1,) + tuple(b"0112")) and b.votes >= 2
    assert isinstance(c, DecodedBarcode) and c.text == "".join(map(str, EAN13_A))
    # the records are the oracles' readings of the very patches predict_patches returns
    _, patches = runner.predict_patches(model, frames, expand=1.25)
    for k in (0, 1):
        assert decoded[k] == text_results_to_records(to.decode_patches(patches[k][None], [1], 0), [1])[0]
    assert decoded[2] == results_to_records(do.decode_patches(patches[2][None], [1], 0), [1])[0]
    only_text = runner.predict_decoded(model, frames, symbologies=4)[1]
    assert [r[0] for r in only_text] == [a, b, None]
    # the default stays the retail family alone: today's results
    found3, decoded3 = runner.predict_decoded(model, frames)
    assert [_key(o) for o in found3] == [_key(o) for o in want_found] and [r[0] for r in decoded3] == [None, None, c]
