"""GPU: ubd_decode_patches (EAN-13 / UPC-A / EAN-8 out of the object patches) against the numpy restatement
tests/decode_oracle.py, which tests/test_decode_host.py pins on rendered symbols.  Every comparison is np.array_equal: no
tolerance.  The result buffer is pre-filled with a sentinel and carries guard bytes at both ends: rows of slots without an
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
from ubdvss_amd import (_lib, NetConfig, Model, ModelRunner, DecodedBarcode, decode_patches_on_device,  # noqa: E402
                        extract_objects_on_device, results_to_records)

pytestmark = pytest.mark.gpu

SENT, GUARD = 0xA5, 64
SENT32 = int(np.frombuffer(bytes([SENT] * 4), np.int32)[0])
NONE = [0, 0, 0] + [-1] * 13
EAN13_A, UPC_A, EAN13_B = (dc.with_check(b) for b in ([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3], [0, 3, 6, 0, 0, 0, 2, 9, 1, 4, 5, 2],
                                                       [9, 7, 8, 1, 8, 6, 1, 9, 7, 2, 7, 1]))
EAN8_A, EAN8_B = dc.with_check([5, 5, 1, 2, 3, 4, 5]), dc.with_check([9, 6, 3, 8, 5, 0, 7])


def _params(**kw):
    merged = dict(do.DEFAULTS, **kw)
    return _lib.UbdDecodeParams(*[merged[k] for k, _ in _lib.UbdDecodeParams._fields_])


def _call(lib, patches_d, counts_d, shape, params, out):
    n, cap, ph, pw, c = shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.ubd_decode_patches(patches_d.data_ptr(), counts_d.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params),
                                  out.data_ptr() + GUARD, st)


def _run_and_check(patches, counts, **kw):
    """one direct call of the C entry point; result rows, untouched rows and guards against the oracle.  Returns the rows."""
    lib = _lib.load()
    patches = np.ascontiguousarray(patches)
    n, cap = patches.shape[:2]
    patches_d, counts_d = torch.from_numpy(patches).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    out = torch.full((2 * GUARD + n * cap * 64,), SENT, dtype=torch.uint8, device="cuda")
    _lib.check(_call(lib, patches_d, counts_d, patches.shape, _params(**kw), out), "ubd_decode_patches")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
    got = got[GUARD:-GUARD].view(np.int32).reshape(n, cap, 16)
    want = do.decode_patches(patches, counts, SENT32, **kw)
    assert np.array_equal(got, want), [(i, j, got[i, j].tolist(), want[i, j].tolist())
                                       for i in range(n) for j in range(cap) if not np.array_equal(got[i, j], want[i, j])]
    return got


def _symbol(h, w, digits, rng=None):
    """the widest upright drawing of the symbol that leaves five modules of quiet zone in w pixels (None: it does not fit)"""
    m = len(dc.modules(digits))
    px = w // (m + 10)
    if px < 1:
        return None
    g = dc.flat_patch([digits], px, h, w, (w - m * px) // 2)[:, :, 0]
    return g if rng is None else _noisy(rng, g)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("ph,pw", [(1, 32), (5, 95), (64, 256), (13, 1024)])
def test_patch_sizes_channels_and_counts(ph, pw, c):
    """n = 3, cap = 2, counts [0, 2, cap + 1]: image 0 holds valid symbols that must not be read"""
    rng = np.random.default_rng(ph * 1000 + pw)
    kinds = [_symbol(ph, pw, EAN13_A, rng), _symbol(ph, pw, EAN8_A, rng), _symbol(ph, pw, EAN13_B), _symbol(ph, pw, EAN8_B)]
    kinds = [k for k in kinds if k is not None] + [_stripes(rng, ph, pw), _stripes(rng, ph, pw, 1, 3), rng.integers(0, 256, (ph, pw), dtype=np.uint8)]
    grey = np.stack([kinds[0], kinds[1], kinds[0], kinds[1][::-1, ::-1], kinds[2], kinds[-1]]).reshape(3, 2, ph, pw)
    got = _run_and_check(_tint(grey, c, seed=pw), [0, 2, 3])
    assert (got[0] == SENT32).all()
    if pw == 256:                                                       # (at 1024 a run is wider than the default window)
        assert got[1, 0, 0] == 13 and got[1, 0, 3:].tolist() == EAN13_A and got[1, 1, 2] == 2      # upright; half-turned


PARAM_SETS = [dict(scan_rows=1, band=0, window=1, contrast=0, min_votes=1), dict(scan_rows=32, band=8, window=64, contrast=255, min_votes=64),
              dict(scan_rows=8, band=8, window=1, contrast=255), dict(scan_rows=32, band=0, window=64, contrast=0, min_votes=1),
              dict(symbologies=1, quiet=0), dict(symbologies=2, quiet=16), dict(scan_rows=1, band=8, window=64, contrast=24, min_votes=2)]


@pytest.fixture(scope="module")
def mixed_patches():
    """64 x 256 x 1: noisy symbols of both families and directions, stripes, noise, a faint symbol (contrast clamp), two payloads"""
    rng = np.random.default_rng(23)
    faint = (128 + (dc.flat_patch([EAN13_A], 2, 64, 256, 33)[:, :, 0].astype(np.int32) - 128) // 16).astype(np.uint8)
    two = np.concatenate([_symbol(64, 256, EAN13_A)[:32], _symbol(64, 256, EAN13_B)[32:]])
    grey = [_symbol(64, 256, EAN13_A, rng), _symbol(64, 256, EAN8_A, rng)[::-1, ::-1], _symbol(64, 256, UPC_A, rng)[::-1, ::-1],
            _symbol(64, 256, EAN8_B, rng), _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8), faint, two]
    return np.stack(grey).reshape(2, 4, 64, 256, 1)


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_parameter_extremes(mixed_patches, kw):
    got = _run_and_check(mixed_patches, [4, 4], **kw)
    if kw == dict(symbologies=1, quiet=0):
        assert got[0, 0, :3].tolist() == [13, 8, 1] and got[0, 1].tolist() == NONE and got[0, 2, 2] == 2 and got[1, 3].tolist() == NONE


def test_defaults_on_the_mixed_patches(mixed_patches):
    got = _run_and_check(mixed_patches, [4, 4])
    assert got[0, 0].tolist() == [13, 8, 1] + EAN13_A and got[0, 1].tolist() == [8, 8, 2] + EAN8_A + [-1] * 5
    assert got[0, 2].tolist() == [13, 8, 2] + UPC_A and got[0, 3, 0] == 8
    assert [got[1, j].tolist() for j in range(4)] == [NONE] * 4          # stripes, noise, below the contrast, a tie of two payloads
    assert _run_and_check(mixed_patches, [4, 4], contrast=2)[1, 2].tolist() == [13, 8, 1] + EAN13_A      # the faint one, once allowed


def test_every_digit_of_every_set_in_one_call():
    """twenty EAN-13 whose left halves hold every digit in set L and in set G, whose right halves every digit in set R, and ten
    EAN-8 (L and R only), upright and half-turned"""
    e13 = [dc.with_check([i % 10] + [(3 * i + 7 * k) % 10 for k in range(11)]) for i in range(20)]
    e8 = [dc.with_check([(i + 3 * k) % 10 for k in range(7)]) for i in range(10)]
    seen = {(p, d) for s in e13 for p, d in zip(dc.PARITY[s[0]], s[1:7])} | {("R", d) for s in e13 for d in s[7:]}
    assert seen == {(p, d) for p in "LGR" for d in range(10)}
    symbols = e13 + e8
    grey = np.stack([_symbol(16, 256, s) if k % 2 else _symbol(16, 256, s)[::-1, ::-1] for k, s in enumerate(symbols)])
    got = _run_and_check(grey.reshape(3, 10, 16, 256, 1), [10, 10, 10], scan_rows=2, band=0)
    for k, s in enumerate(symbols):
        assert got[k // 10, k % 10].tolist() == [len(s), 2, 1 if k % 2 else 2] + s + [-1] * (13 - len(s)), k


def test_the_most_edges_a_line_can_hold():
    """1024 pixels of alternating 1-pixel stripes: 1023 edges, every other one a candidate start of both families, both ways"""
    stripes = np.broadcast_to(np.where(np.arange(1024) % 2, 225, 35).astype(np.uint8)[None, :], (13, 1024))
    e, _ = do.line_edges(do.line_d(*do.line_profile(do.luma(stripes), 0, 8, 1), 16, 24))
    assert len(e) == 1023
    wide = _symbol(13, 1024, EAN13_B)
    patches = np.stack([stripes, stripes[:, ::-1], wide, wide[::-1, ::-1]]).reshape(1, 4, 13, 1024, 1)
    got = _run_and_check(patches, [4])
    assert got[0, 0].tolist() == NONE and got[0, 2].tolist() == [13, 8, 1] + EAN13_B and got[0, 3, 2] == 2
    _run_and_check(patches, [4], scan_rows=32, band=8, window=64, quiet=0, min_votes=1)


def test_two_symbols_side_by_side_the_lowest_start_counts():
    patch = dc.flat_patch([EAN8_A, EAN8_B], 1, 8, 256, 40, gap=20)
    patches = np.stack([patch, patch[::-1, ::-1]]).reshape(1, 2, 8, 256, 1)
    got = _run_and_check(patches, [2], scan_rows=1, min_votes=1)
    assert got[0, 0].tolist() == [8, 1, 1] + EAN8_A + [-1] * 5 and got[0, 1].tolist() == [8, 1, 2] + EAN8_A + [-1] * 5
    got = _run_and_check(patches, [2], scan_rows=5, band=0)
    assert got[0, 0, :3].tolist() == [8, 5, 1]


def test_zero_differences_and_tied_characters():
    """three grey levels under window 1 make d[x] == 0 (a light pixel by the rule); a character drawn halfway between the
    patterns of 1 and 7 ties and rejects its candidate"""
    levels = np.array([35, 130, 225, 130], np.uint8)[np.arange(256) % 4]
    three = np.broadcast_to(levels[None, :], (64, 256))
    d = do.line_d(*do.line_profile(do.luma(three), 0, 8, 1), 1, 0)
    assert d.count(0) >= 100 and min(d) < 0 < max(d)
    digits = dc.with_check([1, 5, 1, 2, 3, 4, 5])
    runs_px = [2 * r for r in dc.runs(digits)]
    exact = np.broadcast_to(_row_from_pixel_runs(runs_px, 256, 40)[None, :], (64, 256))
    assert runs_px[3:7] == [4, 4, 4, 2]                                 # the first character: set L, digit 1
    runs_px[3:7] = [3, 5, 3, 3]
    tied = np.broadcast_to(_row_from_pixel_runs(runs_px, 256, 40)[None, :], (64, 256))
    e, _ = do.line_edges(do.line_d(*do.line_profile(do.luma(tied), 0, 8, 1), 16, 24))
    assert do.decode_character([e[4] - e[3], e[5] - e[4], e[6] - e[5], e[7] - e[6]], "L") is None      # the tie itself
    patches = np.stack([three, three[:, ::-1], exact, tied]).reshape(1, 4, 64, 256, 1)
    _run_and_check(patches, [4], window=1, contrast=0, min_votes=1)
    got = _run_and_check(patches, [4])
    assert got[0, 2].tolist() == [8, 8, 1] + digits + [-1] * 5 and got[0, 3].tolist() == NONE


@pytest.fixture(scope="module")
def rendered():
    """frames with an EAN-13 and an EAN-8 at 3 pixels per module, blurred, noisy and unevenly lit, and their true quads"""
    return [dc.render(EAN13_A, 3, -33.0, seed=5, **dc.HARD), dc.render(EAN8_A, 3, 101.0, seed=6, **dc.HARD)]


def test_rendered_symbols_of_both_families_in_both_directions(rendered):
    grey = []
    for frame, quad in rendered:
        q = dc.int_quad(quad)
        grey += [opo.extract(frame[:, :, None], q, 64, 256, None, 1.25)[0][:, :, 0], opo.extract(frame[:, :, None], q[4:] + q[:4], 64, 256, None, 1.25)[0][:, :, 0]]
    for c in (1, 3):
        got = _run_and_check(_tint(np.stack(grey).reshape(2, 2, 64, 256), c, seed=9), [2, 2])
        for i, digits in enumerate((EAN13_A, EAN8_A)):
            for j in range(2):
                assert got[i, j, 0] == len(digits) and got[i, j, 1] >= 2 and got[i, j, 2] == 1 + j, (c, i, j, got[i, j])
                assert got[i, j, 3:3 + len(digits)].tolist() == digits


def test_graph_capture_equals_the_direct_call(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    params = _params()
    nbytes = 2 * GUARD + 2 * 4 * 64
    direct = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")

    def call(o):
        _lib.check(_call(lib, patches_d, counts_d, mixed_patches.shape, params, o), "ubd_decode_patches")
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
    rows = direct[GUARD:-GUARD].cpu().numpy().view(np.int32).reshape(2, 4, 16)
    assert rows[0, 0, 0] == 13 and (rows[1, 3] == SENT32).all()


def test_refusals_leave_the_results_untouched(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + 2 * 4 * 64,), SENT, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for field, value in (("symbologies", 0), ("scan_rows", 33), ("band", 9), ("window", 0), ("contrast", 256), ("quiet", 17), ("min_votes", 17)):
        p = _params(**{field: value})
        assert _call(lib, patches_d, counts_d, mixed_patches.shape, p, out) != 0
        assert lib.ubd_last_error().decode().startswith("ubd_decode_patches")
    for shape in ((2, 4, 64, 31, 1), (2, 4, 1025, 256, 1), (2, 4, 64, 256, 2), (0, 4, 64, 256, 1), (2, 0, 64, 256, 1)):
        assert _call(lib, patches_d, counts_d, shape, _params(), out) != 0
    assert lib.ubd_decode_patches(None, counts_d.data_ptr(), 2, 4, 64, 256, 1, ctypes.byref(_params()), out.data_ptr() + GUARD, st) != 0
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert _call(lib, patches_d, counts_d, mixed_patches.shape, _params(), out) == 0     # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert (out[GUARD:-GUARD] != SENT).any() and (out[:GUARD] == SENT).all() and (out[-GUARD:] == SENT).all()


def test_python_seam_extract_then_decode(rendered):
    """extract_objects_on_device on the rendered frames with their true quads, then decode_patches_on_device: the encoded digits"""
    frames = [np.repeat(f[:, :, None], 3, axis=2) for f, _ in rendered]
    quads = np.zeros((2, 2, 8), np.int32)
    quads[0, 0], quads[1, 0] = dc.int_quad(rendered[0][1]), dc.int_quad(rendered[1][1])
    quads[1, 1] = quads[1, 0][[4, 5, 6, 7, 0, 1, 2, 3]]
    counts = np.array([1, 2], np.int32)
    patches = extract_objects_on_device(frames, quads, counts, expand=1.25)
    results = decode_patches_on_device(patches, counts)
    assert results.shape == (2, 2, 16) and results.dtype == torch.int32 and results.is_cuda
    want = do.decode_patches(patches.cpu().numpy(), counts, 0)
    assert np.array_equal(results.cpu().numpy(), want)
    records = results_to_records(results, counts)
    assert [len(r) for r in records] == [1, 2]
    text13, text8 = "".join(map(str, EAN13_A)), "".join(map(str, EAN8_A))
    assert records[0][0] == DecodedBarcode("EAN-13", text13, records[0][0].votes, False, False) and records[0][0].votes >= 2
    assert (records[1][0].text, records[1][0].upside_down, records[1][1].text, records[1][1].upside_down) == (text8, False, text8, True)
    only8 = results_to_records(decode_patches_on_device(patches, torch.from_numpy(counts).cuda(), symbologies=2, scan_rows=16), counts)
    assert only8[0][0] is None and only8[1][0].text == text8
    with pytest.raises(TypeError):
        decode_patches_on_device(patches, counts, rows=4)
    with pytest.raises(RuntimeError, match="ubd_decode_patches"):
        decode_patches_on_device(patches, counts, scan_rows=40)


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


def test_predict_decoded_with_the_golden_detection_weights(golden_dir):
    """The golden detection weights are a random initialisation: at pixel_threshold 0.3 every pixel is positive and each frame
    yields one box, its whole frame (tests/test_gpu_object_patches.py).  The frames are upright symbols with quiet zones, so the
    box holds the symbol; what lies outside the frame reads as 0 and ends at the quiet zone."""
    from PIL import Image
    from oracle import net_numpy as onet
    d = np.load(os.path.join(golden_dir, "net_rgb_det.npz"))
    cfg = NetConfig(grey=False, fml_compatible=bool(d["fml"]))
    model = Model(cfg)
    model.set_weights(onet.unflatten_weights(d["params"], 3, 0))
    runner = ModelRunner(cfg, pixel_threshold=0.3, max_objects_per_image=16)
    frames = [dc.flat_patch([EAN13_A], 3, 120, 320, 17, channels=3), Image.fromarray(dc.flat_patch([EAN8_A], 3, 90, 240, 20, channels=3)),
              dc.flat_patch([UPC_A], 3, 120, 320, 17, channels=3)]
    want_found = runner.predict_images(model, frames)
    found, decoded = runner.predict_decoded(model, frames)
    assert [_key(o) for o in found] == [_key(o) for o in want_found]
    assert [len(o) for o in found] == [1, 1, 1] and [len(r) for r in decoded] == [1, 1, 1]
    for rec, digits in zip(decoded, (EAN13_A, EAN8_A, UPC_A)):
        assert rec[0] is not None and rec[0].text == "".join(map(str, digits)) and rec[0].votes >= 2, rec
        assert rec[0].symbology == ("EAN-13" if len(digits) == 13 else "EAN-8") and rec[0].is_upc_a == (digits is UPC_A)
    # the records are the oracle's reading of the very patches predict_patches returns
    _, patches = runner.predict_patches(model, frames, expand=1.25)
    for k in range(3):
        want = results_to_records(do.decode_patches(patches[k][None], [1], 0), [1])[0]
        assert decoded[k] == want
    f1, d1 = runner.predict_decoded(model, frames, patch_size=(32, 384), batch_size=1, scan_rows=4, min_votes=1)
    assert [_key(o) for o in f1] == [_key(o) for o in want_found] and [r[0].text for r in d1] == [r[0].text for r in decoded]
