"""GPU: ubd_decode_width_patches (ITF and Code 39 out of the object patches) against the numpy restatement
tests/width_decode_oracle.py, which tests/test_width_decode_host.py pins on rendered symbols.  Every comparison is np.array_equal:
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
import width_decode_cases as wc  # noqa: E402
import width_decode_oracle as wo  # noqa: E402
from ubdvss_amd import (_lib, NetConfig, Model, ModelRunner, DecodedBarcode, DecodedText, DecodedWidth, decode_width_patches_on_device,  # noqa: E402
                        extract_objects_on_device, results_to_records, text_results_to_records, width_results_to_records)

pytestmark = pytest.mark.gpu

SENT, GUARD, ROW = 0xA5, 64, 128
NONE = [0] * 8 + [0xFF] * 120
GTIN14 = "15400141288763"
EAN13_A = dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])
ITF_A, ITF_B, C39_A, C39_B = ("itf", "123456"), ("itf", "65432109"), ("c39", "AB"), ("c39", "X-9")


def _params(**kw):
    merged = dict(wo.DEFAULTS, **kw)
    return _lib.UbdDecodeParams(*[merged[k] for k, _ in _lib.UbdDecodeParams._fields_])


def _call(lib, patches_d, counts_d, shape, params, out):
    n, cap, ph, pw, c = shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.ubd_decode_width_patches(patches_d.data_ptr(), counts_d.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params),
                                        out.data_ptr() + GUARD, st)


def _row(symbol, votes, mask):
    """the result row of a symbol (kind, text) read with ``votes`` votes, from what was encoded and the oracle's check rule"""
    kind, text = symbol
    code, elements = (25 if kind == "itf" else 39), [ord(ch) for ch in text]
    return [code, votes, mask, len(elements), int(wo.check_holds(code, elements)), 0, 0, 0] + elements + [0xFF] * (120 - len(elements))


_EDGES = {}                                                             # (patch bytes, shape, scan parameters) -> the edge lists of its scan lines


def _edges(patch, scan_rows, band, window, contrast):
    """the scan front end of the oracle costs most of its time and does not depend on the symbologies: computed once per
    (patch, scan parameters) and shared by the calls that differ in the rest"""
    key = (patch.tobytes(), patch.shape, scan_rows, band, window, contrast)
    if key not in _EDGES:
        lum = do.luma(patch)
        _EDGES[key] = [do.line_edges(do.line_d(*do.line_profile(lum, k, scan_rows, band), window, contrast)) for k in range(scan_rows)]
    return _EDGES[key]


def _want(patches, counts, **kw):
    """wo.decode_patches(patches, counts, SENT, **kw) through the shared edge lists (test_the_shared_reference_is_the_oracle)"""
    p = dict(wo.DEFAULTS, **kw)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, ROW), SENT, np.uint8)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            votes = []
            for e, l2d in _edges(patches[i, j], p["scan_rows"], p["band"], p["window"], p["contrast"]):
                votes += wo.line_votes(e, l2d, patches.shape[3], p["symbologies"], p["quiet"])
            out[i, j] = wo.tally(votes, p["min_votes"])
    return out


def _run_and_check(patches, counts, **kw):
    """one direct call of the C entry point; result rows, untouched rows and guards against the oracle.  Returns the rows."""
    lib = _lib.load()
    patches = np.ascontiguousarray(patches)
    n, cap = patches.shape[:2]
    patches_d, counts_d = torch.from_numpy(patches).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    out = torch.full((2 * GUARD + n * cap * ROW,), SENT, dtype=torch.uint8, device="cuda")
    _lib.check(_call(lib, patches_d, counts_d, patches.shape, _params(**kw), out), "ubd_decode_width_patches")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
    got = got[GUARD:-GUARD].reshape(n, cap, ROW)
    want = _want(patches, counts, **kw)
    assert np.array_equal(got, want), [(i, j, got[i, j, :24].tolist(), want[i, j, :24].tolist())
                                       for i in range(n) for j in range(cap) if not np.array_equal(got[i, j], want[i, j])]
    return got


def _modules(symbol, narrow=2, wide=5):
    return (wc.itf_modules if symbol[0] == "itf" else wc.c39_modules)(symbol[1], narrow, wide)


def _symbol(h, w, symbol, rng=None):
    """the widest upright drawing of the symbol, in half-narrow units at a ratio of 2.5, that leaves five narrow runs of quiet
    zone in w pixels; where not even one pixel per unit fits, narrow 1 and wide 2 pixels (None: that does not fit either)"""
    mods = _modules(symbol)
    px = w // (len(mods) + 20)
    if px < 1:
        mods, px = _modules(symbol, 1, 2), 1
        if len(mods) + 10 > w:
            return None
    g = wc.flat_patch([mods], px, h, w, (w - len(mods) * px) // 2)[:, :, 0]
    return g if rng is None else _noisy(rng, g)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("ph,pw", [(1, 32), (5, 95), (64, 256), (13, 1024)])
def test_patch_sizes_channels_and_counts(ph, pw, c):
    """n = 2, cap = 4, counts [0, 3]: image 0 is empty though its slots hold valid symbols, which must not be read, image 1 is
    partly filled.  At width 32 no symbol fits (the shortest, a Code 39 of one character, is 38 pixels) and the call runs all the
    same; at 95 both short symbols fit at one pixel per narrow run"""
    rng = np.random.default_rng(ph * 1000 + pw)
    kinds = [_symbol(ph, pw, ITF_A, rng), _symbol(ph, pw, C39_A, rng), _symbol(ph, pw, ITF_B), _symbol(ph, pw, C39_B)]
    assert (kinds[0] is None) == (pw == 32)
    kinds = [k for k in kinds if k is not None] + [_stripes(rng, ph, pw), _stripes(rng, ph, pw, 1, 3), rng.integers(0, 256, (ph, pw), dtype=np.uint8)]
    grey = np.stack([kinds[0], kinds[1], kinds[0], kinds[1], kinds[0], kinds[1][::-1, ::-1], kinds[2], kinds[-1]]).reshape(2, 4, ph, pw)
    got = _run_and_check(_tint(grey, c, seed=pw), [0, 3])
    assert (got[0] == SENT).all() and (got[1, 3] == SENT).all()
    if pw in (95, 256):                                                 # (at 1024 a run is wider than the default window)
        assert got[1, 0].tolist() == _row(ITF_A, 8, 1) and got[1, 1].tolist() == _row(C39_A, 8, 2)     # upright; half-turned


# the seven parameter-extreme sets of tests/test_gpu_decode.py; each runs with symbologies 8, 16 and 24
PARAM_SETS = [dict(scan_rows=1, band=0, window=1, contrast=0, min_votes=1), dict(scan_rows=32, band=8, window=64, contrast=255, min_votes=64),
              dict(scan_rows=8, band=8, window=1, contrast=255), dict(scan_rows=32, band=0, window=64, contrast=0, min_votes=1),
              dict(quiet=0), dict(quiet=16), dict(scan_rows=1, band=8, window=64, contrast=24, min_votes=2)]


@pytest.fixture(scope="module")
def mixed_patches():
    """64 x 256 x 1: noisy symbols of both symbologies and directions, stripes, noise, a faint symbol (contrast clamp), two payloads"""
    rng = np.random.default_rng(23)
    faint = (128 + (_symbol(64, 256, ITF_A).astype(np.int32) - 128) // 16).astype(np.uint8)
    two = np.concatenate([_symbol(64, 256, C39_A)[:32], _symbol(64, 256, C39_B)[32:]])
    grey = [_symbol(64, 256, ITF_A, rng), _symbol(64, 256, C39_A, rng)[::-1, ::-1], _symbol(64, 256, ITF_B, rng)[::-1, ::-1],
            _symbol(64, 256, C39_B, rng), _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8), faint, two]
    return np.stack(grey).reshape(2, 4, 64, 256, 1)


def test_the_shared_reference_is_the_oracle(mixed_patches):
    for kw in (dict(), dict(symbologies=8, quiet=0, min_votes=1)):
        assert np.array_equal(_want(mixed_patches, [4, 3], **kw), wo.decode_patches(mixed_patches, [4, 3], SENT, **kw))


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_parameter_extremes(mixed_patches, kw):
    for symbologies in (8, 16, 24):
        got = _run_and_check(mixed_patches, [4, 4], symbologies=symbologies, **kw)
        if kw == dict(quiet=0):
            assert got[0, 0].tolist() == (_row(ITF_A, 8, 1) if symbologies & 8 else NONE)
            assert got[0, 1].tolist() == (_row(C39_A, 8, 2) if symbologies & 16 else NONE) and got[1, 3].tolist() == NONE


def test_defaults_on_the_mixed_patches(mixed_patches):
    got = _run_and_check(mixed_patches, [4, 4])
    assert [got[0, j].tolist() for j in range(4)] == [_row(ITF_A, 8, 1), _row(C39_A, 8, 2), _row(ITF_B, 8, 2), _row(C39_B, 8, 1)]
    assert [got[1, j].tolist() for j in range(4)] == [NONE] * 4          # stripes, noise, below the contrast, a tie of two payloads
    assert _run_and_check(mixed_patches, [4, 4], contrast=2)[1, 2].tolist() == _row(ITF_A, 8, 1)       # the faint one, once allowed


def test_every_character_and_every_pair_in_one_call():
    """all 43 Code 39 characters in one symbol and once more in reverse order, the four with wide spaces alone, and the hundred
    ITF pairs 00..99 in four symbols of 25 (symbol k holds the pairs k, k + 4, ..), at narrow 1 and wide 3 pixels, upright and
    half-turned in turn.  (The pairs in rising order would not do: 00 01 02 .. holds the four narrow runs of a start, and read
    backwards from there the oracle finds a short second ITF, 37383136, whose votes tie with the symbol's: the rules' answer to
    that is "none", on the device as well -- test_a_short_symbol_inside_a_long_one_read_backwards.)"""
    chars = wc.C39_CHARS[:43]
    pairs = ["".join(f"{v:02d}" for v in range(k, 100, 4)) for k in range(4)]
    symbols = [("c39", chars), ("c39", chars[::-1]), ("c39", "$/+%"), ("itf", GTIN14)] + [("itf", p) for p in pairs]
    assert {s[1][k:k + 2] for s in symbols[4:] for k in range(0, 50, 2)} == {f"{v:02d}" for v in range(100)}
    grey = []
    for k, s in enumerate(symbols):
        mods = _modules(s, 1, 3)
        g = wc.flat_patch([mods], 1, 8, 1024, (1024 - len(mods)) // 2)[:, :, 0]
        grey.append(g if k % 2 else g[::-1, ::-1])
    got = _run_and_check(np.stack(grey).reshape(2, 4, 8, 1024, 1), [4, 4], scan_rows=2, band=0)
    for k, s in enumerate(symbols):
        assert got[k // 4, k % 4].tolist() == _row(s, 2, 1 if k % 2 else 2), k
    assert got[0, 3, 4] == 1 and got[0, 0, 3] == 43 and got[1, 0, 3] == 50


def test_a_short_symbol_inside_a_long_one_read_backwards():
    """ITF has no start that data cannot imitate: the pairs 00 01 .. 24 read right to left hold a valid ITF of four pairs.  Both
    payloads get one vote per line, so the row is "none" (callers of ITF fix the length they expect: INTEGRATION.md)"""
    digits = "".join(f"{v:02d}" for v in range(25))
    mods = wc.itf_modules(digits, 1, 3)
    g = wc.flat_patch([mods], 1, 8, 1024, (1024 - len(mods)) // 2)[:, :, 0]
    e, l2d = do.line_edges(do.line_d(*do.line_profile(do.luma(g), 0, 2, 0), 16, 24))
    assert wo.line_votes(e, l2d, 1024, 24, 3) == [(1, 25, tuple(digits.encode())), (2, 25, tuple(b"37383136"))]
    got = _run_and_check(np.stack([g, g[::-1, ::-1]]).reshape(1, 2, 8, 1024, 1), [2], scan_rows=2, band=0)
    assert got[0, 0].tolist() == NONE and got[0, 1].tolist() == NONE


def test_the_length_limits_and_the_most_edges_a_line_can_hold():
    """30 pairs and 60 characters are read, 31 and 61 are one too many; 1024 pixels of alternating 1-pixel stripes are 1023
    edges, every other one a candidate start, both ways"""
    rng = np.random.default_rng(3)
    digits = "".join(map(str, rng.integers(0, 10, 62)))
    chars = "".join(wc.C39_CHARS[int(v)] for v in rng.integers(0, 43, 61))
    stripes = np.broadcast_to(np.where(np.arange(1024) % 2, 225, 35).astype(np.uint8)[None, :], (13, 1024))
    e, _ = do.line_edges(do.line_d(*do.line_profile(do.luma(stripes), 0, 8, 1), 16, 24))
    assert len(e) == 1023
    symbols = [("itf", digits[:60]), ("itf", digits), ("c39", chars[:60]), ("c39", chars)]
    grey = []
    for s in symbols:
        mods = _modules(s, 1, 2)
        grey.append(wc.flat_patch([mods], 1, 13, 1024, (1024 - len(mods)) // 2)[:, :, 0])
    patches = np.stack(grey + [stripes, stripes[:, ::-1]]).reshape(1, 6, 13, 1024, 1)
    got = _run_and_check(patches, [6])
    assert got[0, 0].tolist() == _row(symbols[0], 8, 1) and got[0, 2].tolist() == _row(symbols[2], 8, 1) and got[0, 0, 3] == got[0, 2, 3] == 60
    assert [got[0, j].tolist() for j in (1, 3, 4, 5)] == [NONE] * 4
    _run_and_check(patches, [6], scan_rows=32, band=8, window=64, quiet=0, min_votes=1)


def test_two_symbols_side_by_side_the_lowest_start_counts():
    a, b, c = _modules(ITF_A), _modules(("itf", "654321")), _modules(C39_A)
    patch = wc.flat_patch([a, b], 1, 8, 512, 30, gap=20)
    mixed = wc.flat_patch([a, c], 1, 8, 512, 30, gap=30)
    patches = np.stack([patch, patch[::-1, ::-1], mixed, mixed[::-1, ::-1]]).reshape(1, 4, 8, 512, 1)
    got = _run_and_check(patches, [4], scan_rows=1, min_votes=1)
    assert got[0, 0].tolist() == _row(ITF_A, 1, 1) and got[0, 1].tolist() == _row(ITF_A, 1, 2)
    assert got[0, 2].tolist() == NONE                                    # one vote for each symbology's symbol: a tie
    got = _run_and_check(patches, [4], scan_rows=5, band=0)
    assert got[0, 0, :3].tolist() == [25, 5, 1] and got[0, 2].tolist() == NONE
    assert _run_and_check(patches, [4], symbologies=16)[0, 2].tolist() == _row(C39_A, 8, 1)
    assert _run_and_check(patches, [4], symbologies=8)[0, 3].tolist() == _row(ITF_A, 8, 2)


def _flat(runs_px, start=40):
    return np.broadcast_to(_row_from_pixel_runs(runs_px, 512, start)[None, :], (64, 512))


def test_rejections_and_tie():
    """a dark bar two narrow runs before the symbol (QZ = 3); a Code 39 gap wider than half a character; a character and a pair
    drawn 1.22 times as wide as their neighbours; a character with two and one with four wide runs; two ITF pairs; two payloads
    with four lines each; and the same symbols drawn right, which are read"""
    itf, c39 = wc.itf_runs("123456", 4, 10), wc.c39_runs("AB", 4, 10)
    two, four = list(c39), list(c39)
    two[10 + c39[10:19].index(10)] = 4                                  # in the character A
    four[10 + c39[10:19].index(4)] = 10
    tie = np.concatenate([_flat(itf)[:32], _flat(wc.itf_runs("654321", 4, 10))[32:]])
    bad = [_flat([6, 8] + itf, 20), _flat(c39 + [8, 6]), _flat(wc.c39_runs("AB", 4, 10, gap=28)), _flat(c39[:20] + wc.c39_runs("AB", 5, 12)[20:]),
           _flat(itf[:24] + wc.itf_runs("123456", 5, 12)[24:]), _flat(two), _flat(four), _flat(wc.itf_runs("1234", 4, 10)), tie]
    good = [_flat([6, 16] + itf, 20), _flat(c39 + [16, 6]), _flat(wc.c39_runs("AB", 4, 10, gap=27)), _flat(itf), _flat(c39),
            _flat(wc.itf_runs("123410", 4, 10))]                        # the last: data before stop
    patches = np.stack(bad + good + [bad[0]]).reshape(2, 8, 64, 512, 1)
    got = _run_and_check(patches, [8, 7])
    rows = [got[k // 8, k % 8].tolist() for k in range(15)]
    assert rows[:9] == [NONE] * 9
    assert rows[9:] == [_row(ITF_A, 8, 1), _row(C39_A, 8, 1), _row(C39_A, 8, 1), _row(ITF_A, 8, 1), _row(C39_A, 8, 1), _row(("itf", "123410"), 8, 1)]
    got = _run_and_check(patches, [8, 7], min_votes=1, quiet=0)
    assert got[0, 0].tolist() == _row(ITF_A, 8, 1) and [got[0, j].tolist() for j in range(2, 8)] == [NONE] * 6


@pytest.fixture(scope="module")
def rendered():
    """frames with an ITF-14 at 3 pixels per narrow run and a ratio of 2.5 and a Code 39 at 2 pixels and a ratio of 3, blurred,
    noisy and unevenly lit, and their true quads"""
    itf, c39 = ("itf", GTIN14), ("c39", "CODE 39R")
    return [(itf, ) + wc.render(_modules(itf, 2, 5), 1.5, -33.0, seed=5, **dc.HARD), (c39, ) + wc.render(_modules(c39, 2, 6), 1.0, 101.0, seed=6, **dc.HARD)]


def test_rendered_symbols_in_both_directions(rendered):
    grey = []
    for _, frame, quad in rendered:
        q = dc.int_quad(quad)
        grey += [opo.extract(frame[:, :, None], q, 64, 512, None, 1.25)[0][:, :, 0], opo.extract(frame[:, :, None], q[4:] + q[:4], 64, 512, None, 1.25)[0][:, :, 0]]
    for c in (1, 3):
        got = _run_and_check(_tint(np.stack(grey).reshape(2, 2, 64, 512), c, seed=9), [2, 2])
        for i, (symbol, _, _) in enumerate(rendered):
            for j in range(2):
                assert got[i, j, 1] >= 2 and got[i, j].tolist() == _row(symbol, int(got[i, j, 1]), 1 + j), (c, i, j, got[i, j, :8])
                assert got[i, j, 4] == 1                                 # both carry their check character


def test_graph_capture_equals_the_direct_call(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    params = _params()
    nbytes = 2 * GUARD + 2 * 4 * ROW
    direct = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")

    def call(o):
        _lib.check(_call(lib, patches_d, counts_d, mixed_patches.shape, params, o), "ubd_decode_width_patches")
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
    assert rows[0, 0, 0] == 25 and rows[0, 1, 0] == 39 and (rows[1, 3] == SENT).all()


def test_refusals_leave_the_results_untouched(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + 2 * 4 * ROW,), SENT, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for field, value in (("symbologies", 0), ("symbologies", 1), ("symbologies", 4), ("symbologies", 7), ("symbologies", 9), ("symbologies", 32),
                         ("symbologies", -1), ("scan_rows", 0), ("scan_rows", 33), ("band", -1), ("band", 9), ("window", 0), ("window", 65),
                         ("contrast", -1), ("contrast", 256), ("quiet", -1), ("quiet", 17), ("min_votes", 0), ("min_votes", 17)):
        p = _params(**{field: value})
        assert _call(lib, patches_d, counts_d, mixed_patches.shape, p, out) != 0, (field, value)
        assert lib.ubd_last_error().decode().startswith("ubd_decode_width_patches")
    for shape in ((2, 4, 64, 31, 1), (2, 4, 64, 1025, 1), (2, 4, 1025, 256, 1), (2, 4, 0, 256, 1), (2, 4, 64, 256, 2), (0, 4, 64, 256, 1), (2, 0, 64, 256, 1)):
        assert _call(lib, patches_d, counts_d, shape, _params(), out) != 0
    good = [patches_d.data_ptr(), counts_d.data_ptr(), 2, 4, 64, 256, 1, ctypes.byref(_params()), out.data_ptr() + GUARD, st]
    for k in (0, 1, 7, 8):                                              # a null pointer in each pointer's place
        assert lib.ubd_decode_width_patches(*[None if q == k else a for q, a in enumerate(good)]) != 0
    for off in (1, 2, 3):                                               # rows leave as dwords
        assert lib.ubd_decode_width_patches(*good[:8], out.data_ptr() + GUARD + off, st) != 0
    torch.cuda.synchronize()
    assert (out == SENT).all()
    for symbologies in (8, 16, 24):                                     # and the three values it takes are accepted
        assert _call(lib, patches_d, counts_d, mixed_patches.shape, _params(symbologies=symbologies), out) == 0
    torch.cuda.synchronize()
    assert (out[GUARD:-GUARD] != SENT).any() and (out[:GUARD] == SENT).all() and (out[-GUARD:] == SENT).all()


def test_python_seam_extract_then_decode(rendered):
    """extract_objects_on_device on the rendered frames with their true quads, then decode_width_patches_on_device: what was encoded"""
    frames = [np.repeat(f[:, :, None], 3, axis=2) for _, f, _ in rendered]
    quads = np.zeros((2, 2, 8), np.int32)
    quads[0, 0], quads[1, 0] = dc.int_quad(rendered[0][2]), dc.int_quad(rendered[1][2])
    quads[1, 1] = quads[1, 0][[4, 5, 6, 7, 0, 1, 2, 3]]
    counts = np.array([1, 2], np.int32)
    patches = extract_objects_on_device(frames, quads, counts, patch_size=(64, 512), expand=1.25)
    results = decode_width_patches_on_device(patches, counts)
    assert results.shape == (2, 2, 128) and results.dtype == torch.uint8 and results.is_cuda
    want = wo.decode_patches(patches.cpu().numpy(), counts, 0)
    want[0, 1, 8:] = 0xFF                                               # the empty slot reads as "none"
    assert np.array_equal(results.cpu().numpy(), want)
    records = width_results_to_records(results, counts)
    assert [len(r) for r in records] == [1, 2]
    itf, c39 = records[0][0], records[1][0]
    assert itf == DecodedWidth("ITF", GTIN14, itf.votes, False, True) and itf.votes >= 2
    assert c39 == DecodedWidth("Code 39", "CODE 39R", c39.votes, False, True) and c39.votes >= 2
    assert records[1][1] == c39._replace(upside_down=True, votes=records[1][1].votes)
    only = width_results_to_records(decode_width_patches_on_device(patches, torch.from_numpy(counts).cuda(), scan_rows=16, symbologies=16), counts)
    assert only[0][0] is None and only[1][0].text == "CODE 39R" and only[1][1].upside_down
    with pytest.raises(TypeError):
        decode_width_patches_on_device(patches, counts, rows=4)
    with pytest.raises(RuntimeError, match="ubd_decode_width_patches"):
        decode_width_patches_on_device(patches, counts, symbologies=7)


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


def test_predict_decoded_with_the_golden_detection_weights(golden_dir):
    """The golden detection weights are a random initialisation: at pixel_threshold 0.3 every pixel is positive and each frame
    yields one box, its whole frame (tests/test_gpu_object_patches.py).  The frames are upright symbols with quiet zones, one of
    every family: an EAN-13, a Code 128, an ITF and a Code 39."""
    from oracle import net_numpy as onet
    d = np.load(os.path.join(golden_dir, "net_rgb_det.npz"))
    cfg = NetConfig(grey=False, fml_compatible=bool(d["fml"]))
    model = Model(cfg)
    model.set_weights(onet.unflatten_weights(d["params"], 3, 0))
    runner = ModelRunner(cfg, pixel_threshold=0.3, max_objects_per_image=16)
    itf, c39 = _modules(ITF_A, 3, 8), _modules(C39_A, 3, 8)
    frames = [dc.flat_patch([EAN13_A], 3, 120, 320, 17, channels=3), tc.flat_patch([tc.encode_text("UBD1")], 3, 120, 320, 40, channels=3),
              wc.flat_patch([itf], 1, 120, 320, (320 - len(itf)) // 2, channels=3), wc.flat_patch([c39], 1, 120, 320, (320 - len(c39)) // 2, channels=3)]
    want_found = runner.predict_images(model, frames)
    found, decoded = runner.predict_decoded(model, frames, symbologies=31)
    assert [_key(o) for o in found] == [_key(o) for o in want_found]
    assert [len(o) for o in found] == [1, 1, 1, 1] and [len(r) for r in decoded] == [1, 1, 1, 1]
    a, b, c, e = (r[0] for r in decoded)
    # (which long side of the whole-frame box lands on top is the extraction's choice: upside_down is the oracle's to say, below)
    assert isinstance(a, DecodedBarcode) and a.text == "".join(map(str, EAN13_A))
    assert isinstance(b, DecodedText) and b.text == "UBD1"
    assert isinstance(c, DecodedWidth) and (c.symbology, c.text, c.checked) == ("ITF", "123456", False) and c.votes >= 2
    assert isinstance(e, DecodedWidth) and (e.symbology, e.text, e.checked) == ("Code 39", "AB", False) and e.votes >= 2
    # the records are the oracles' readings of the very patches predict_patches returns
    _, patches = runner.predict_patches(model, frames, expand=1.25)
    assert decoded[0] == results_to_records(do.decode_patches(patches[0][None], [1], 0), [1])[0]
    assert decoded[1] == text_results_to_records(to.decode_patches(patches[1][None], [1], 0), [1])[0]
    for k in (2, 3):
        assert decoded[k] == width_results_to_records(wo.decode_patches(patches[k][None], [1], 0), [1])[0]
    assert [r[0] for r in runner.predict_decoded(model, frames, symbologies=24)[1]] == [None, None, c, e]
    assert [r[0] for r in runner.predict_decoded(model, frames, symbologies=8 | 4)[1]] == [None, b, c, None]
    assert [r[0] for r in runner.predict_decoded(model, frames, symbologies=7)[1]] == [a, b, None, None]
    assert [r[0] for r in runner.predict_decoded(model, frames)[1]] == [a, None, None, None]      # the default stays the retail family alone
    for value in (32, 63, -1):
        with pytest.raises(ValueError):
            runner.predict_decoded(model, frames, symbologies=value)
