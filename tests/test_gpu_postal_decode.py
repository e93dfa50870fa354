"""GPU: ubd_decode_postal_patches (POSTNET, PLANET, RM4SCC, KIX) against the numpy restatement tests/postal_decode_oracle.py, which
tests/test_postal_decode_host.py pins on rendered symbols.  Every comparison is np.array_equal: no tolerance.  The result
buffer is pre-filled with a sentinel and carries guards at both ends: rows of slots without an object and the guards must keep
it."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
from decode_cases import _stripes, _tint  # noqa: E402
import extra_decode_cases as xc  # noqa: E402
import postal_decode_cases as pc  # noqa: E402
import postal_decode_oracle as po  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import width_decode_cases as wc  # noqa: E402
from test_gpu_extra_decode import PARAM_SETS  # noqa: E402
from test_postal_decode_host import (KIX_TEXT, NONE128, PLANET_DIGITS, RM_TEXT, TEXTS, acceptance_patches, expected_row)  # noqa: E402,F401
from ubdvss_amd import (_lib, NetConfig, Model, ModelRunner, DecodedBarcode, DecodedPostal, DecodedText, DecodedWidth, kix_half_turned,  # noqa: E402
                        postal_results_to_records)

pytestmark = pytest.mark.gpu

ENTRY = "ubd_decode_postal_patches"
OLDER = {"ubd_decode_patches": (1, 2, 64, 3, 67), "ubd_decode_text_patches": (4, 128, 132), "ubd_decode_width_patches": (8, 16, 256, 24, 280)}
GUARD, ROW, SENT = 64, 128, 0xA5
_SCANNED = {}                                                           # (patch bytes, shape, scan parameters) -> po.scan_lines


def _params(**kw):
    merged = dict(po.DEFAULTS, **kw)
    return _lib.UbdDecodeParams(*[merged[k] for k, _ in _lib.UbdDecodeParams._fields_])


def _want(patches, counts, **kw):
    """po.decode_patches(patches, counts, SENT, **kw), the scan front end shared between the masks of one patch"""
    p = dict(po.DEFAULTS, **kw)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, ROW), SENT, np.uint8)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            key = (patches[i, j].tobytes(), patches[i, j].shape, p["scan_rows"], p["band"], p["window"], p["contrast"])
            if key not in _SCANNED:
                _SCANNED[key] = po.scan_lines(patches[i, j], p["scan_rows"], p["band"], p["window"], p["contrast"])
            out[i, j] = po.decode_lines(_SCANNED[key], p["symbologies"], p["window"], p["contrast"], p["quiet"], p["min_votes"])
    return out


def _call(lib, patches_d, counts_d, shape, params, out, entry=ENTRY, offset=GUARD):
    n, cap, ph, pw, c = shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return getattr(lib, entry)(patches_d.data_ptr() if patches_d is not None else None, counts_d.data_ptr() if counts_d is not None else None,
                               n, cap, ph, pw, c, ctypes.byref(params) if params is not None else None,
                               out.data_ptr() + offset if out is not None else None, st)


def _run_and_check(patches, counts, **kw):
    """one direct call of the entry point; result rows, untouched rows and guards against the oracle.  Returns the rows."""
    lib = _lib.load()
    patches = np.ascontiguousarray(patches)
    n, cap = patches.shape[:2]
    patches_d, counts_d = torch.from_numpy(patches).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    out = torch.full((2 * GUARD + n * cap * ROW,), SENT, dtype=torch.uint8, device="cuda")
    _lib.check(_call(lib, patches_d, counts_d, patches.shape, _params(**kw), out), ENTRY)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
    got = got[GUARD:-GUARD].reshape(n, cap, ROW)
    want = _want(patches, counts, **kw)
    assert np.array_equal(got, want), [(i, j, got[i, j, :24].tolist(), want[i, j, :24].tolist())
                                       for i in range(n) for j in range(cap) if not np.array_equal(got[i, j], want[i, j])]
    return got


def _mixed(rng):
    """eight grey 64 x 256 patches: one symbol of every kind, a half-turned RM4SCC and a half-turned POSTNET, stripes and noise"""
    rm, kix = pc.rm4scc_bars(RM_TEXT), pc.kix_bars(KIX_TEXT)
    postnet, planet = pc.postnet_bars("80122"), pc.planet_bars(PLANET_DIGITS)
    return [pc.render(postnet, 5.0, 2.0, noise=4.0, seed=1)[:, :, 0], pc.render(planet, 4.0, 2.0)[:, :, 0], pc.render(rm, 5.0, 2.0, blur=0.6)[:, :, 0],
            pc.render(kix, 5.0, 2.0, angle=1)[:, :, 0], pc.render(rm, 6.0, 3.0, turned=True)[:, :, 0], pc.render(postnet, 6.0, 3.0, turned=True)[:, :, 0],
            _stripes(rng, 64, 256), rng.integers(0, 256, (64, 256), dtype=np.uint8)]


@pytest.fixture(scope="module")
def mixed_patches():
    return np.stack(_mixed(np.random.default_rng(31))).reshape(2, 4, 64, 256, 1)


SHORT_ZIP = "80122" + str(pc.postnet_check("80122"))                    # a POSTNET of 32 bars
MIXED_READS = [(po.POSTNET, SHORT_ZIP, 1), (po.PLANET, TEXTS[po.PLANET], 1), (po.RM4SCC, TEXTS[po.RM4SCC], 1), (po.KIX, KIX_TEXT, 1),
               (po.RM4SCC, TEXTS[po.RM4SCC], 2), (po.POSTNET, SHORT_ZIP, 2)]


def test_the_shared_reference_is_the_oracle(mixed_patches):
    for kw in (dict(), dict(symbologies=po.RM4SCC | po.PLANET, scan_rows=16, quiet=0, min_votes=1)):
        assert np.array_equal(_want(mixed_patches, [4, 3], **kw), po.decode_patches(mixed_patches, [4, 3], SENT, **kw))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("sym", [po.POSTNET, po.PLANET, po.RM4SCC, po.KIX])
def test_the_acceptance_set(acceptance_patches, sym, c):  # noqa: F811
    """the patches of tests/test_postal_decode_host.py of one kind, grey or tinted, under the full mask at scan_rows 16, batched as
    (n, 4) with three objects an image: the device reads each as the oracle does, which is as it was drawn, and leaves the
    fourth slot alone"""
    mine = [m for m in acceptance_patches if m[0] == sym]
    for pw in sorted({m[3].shape[1] for m in mine}):
        sized = [m for m in mine if m[3].shape[1] == pw]
        sized += [sized[-1]] * (-len(sized) % 3)
        grey = np.zeros((len(sized) // 3, 4, 64, pw), np.uint8)
        for k, m in enumerate(sized):
            grey[k // 3, k % 3] = m[3][:, :, 0]
        got = _run_and_check(_tint(grey, c, seed=pw), [3] * (len(sized) // 3), scan_rows=16)
        assert (got[:, 3] == SENT).all()
        for k, (_, text, mask, _) in enumerate(sized):
            r = got[k // 3, k % 3].tolist()
            assert r[1] >= 2 and r == expected_row(sym, text, r[1], mask), (sym, pw, k, r[:12])


@pytest.mark.parametrize("c", [1, 3])
def test_mixed_patches_under_every_mask(mixed_patches, c):
    """the fifteen subsets of 15360 at scan_rows 16; counts [4, 3]: the last slot is not written.  A symbol is read exactly under
    the masks that hold its bit"""
    patches = _tint(mixed_patches[..., 0], c, seed=5)
    for bits in itertools.chain.from_iterable(itertools.combinations((po.POSTNET, po.PLANET, po.RM4SCC, po.KIX), r) for r in range(1, 5)):
        mask = sum(bits)
        got = _run_and_check(patches, [4, 3], symbologies=mask, scan_rows=16)
        assert (got[1, 3] == SENT).all()
        for k, (sym, text, direction) in enumerate(MIXED_READS):
            r = got[k // 4, k % 4].tolist()
            if sym & mask:
                assert r == expected_row(sym, text, r[1], direction) and r[1] >= 2, (mask, k, r[:12])
            else:
                assert r == NONE128, (mask, k, r[:12])
        assert got[1, 2].tolist() == NONE128


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_parameter_extremes(mixed_patches, kw):
    for symbologies in (po.MASK, po.RM4SCC, po.POSTNET | po.KIX):
        _run_and_check(mixed_patches, [4, 4], symbologies=symbologies, **kw)


def test_small_odd_and_wide_patches():
    """1 x 32 and 5 x 64 hold no symbol and run all the same (bars of 5 rows give chains); 64 x 1024: an RM4SCC of 122 bars, the
    longest chain, reads, and a KIX of 124 bars is one of more than 122"""
    rng = np.random.default_rng(5)
    tiny = rng.integers(0, 256, (2, 2, 1, 32, 3), dtype=np.uint8)
    assert (_run_and_check(tiny, [1, 0], min_votes=1)[1] == SENT).all()
    low = [pc.render(pc.kix_bars("12AB"), 3.0, 1.5, h=5, w=64)[:, :, 0], _stripes(rng, 5, 64, 1, 3), rng.integers(0, 256, (5, 64), dtype=np.uint8),
           pc.render(pc.postnet_bars("1")[:10], 4.0, 2.0, h=5, w=64, height=1.0)[:, :, 0]]
    got = _run_and_check(_tint(np.stack(low).reshape(2, 2, 5, 64), 3, seed=3), [2, 1], scan_rows=5, band=0, min_votes=1, quiet=0)
    assert (got[1, 1] == SENT).all()
    long = "".join(po.ALPHABET[int(v)] for v in rng.integers(0, 36, 29))
    wide = [pc.render(pc.rm4scc_bars(long), 8.0, 3.0, w=1024)[:, :, 0], pc.render(pc.kix_bars(long + "12"), 8.0, 3.0, w=1024)[:, :, 0]]
    got = _run_and_check(np.stack(wide).reshape(1, 2, 64, 1024, 1), [2], scan_rows=16)
    r = got[0, 0].tolist()
    assert r == expected_row(po.RM4SCC, long + pc.rm4scc_check(long), r[1], 1) and r[5] == 122 and r[1] >= 2
    assert got[0, 1].tolist() == NONE128


def test_graph_capture_equals_the_direct_call(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    params = _params(scan_rows=16)
    nbytes = 2 * GUARD + 2 * 4 * ROW
    direct = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")

    def call(o):
        _lib.check(_call(lib, patches_d, counts_d, mixed_patches.shape, params, o), ENTRY)
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
    assert [int(v) for v in rows[0, :, 0]] == [80, 76, 82, 75] and (rows[1, 3] == SENT).all()


def test_refusals_leave_the_results_untouched(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + 2 * 4 * ROW,), SENT, dtype=torch.uint8, device="cuda")
    shape = mixed_patches.shape
    older = tuple(v for vs in OLDER.values() for v in vs)
    for value in (0, 32, 512, 479, 16384, -1, 15360 | 512, 15360 | 1, 1024 | 16384) + older:
        assert _call(lib, patches_d, counts_d, shape, _params(symbologies=value), out) != 0, value
        assert lib.ubd_last_error().decode().startswith(ENTRY) and "symbologies" in lib.ubd_last_error().decode()
    for field, value in (("scan_rows", 0), ("scan_rows", 33), ("band", -1), ("band", 9), ("window", 0), ("window", 65), ("contrast", -1),
                         ("contrast", 256), ("quiet", -1), ("quiet", 17), ("min_votes", 0), ("min_votes", 17)):
        assert _call(lib, patches_d, counts_d, shape, _params(**{field: value}), out) != 0, (field, value)
        assert lib.ubd_last_error().decode().startswith(ENTRY) and field in lib.ubd_last_error().decode()
    for bad in ((2, 4, 64, 31, 1), (2, 4, 64, 1025, 1), (2, 4, 1025, 256, 1), (2, 4, 0, 256, 1), (2, 4, 64, 256, 2), (0, 4, 64, 256, 1), (2, 0, 64, 256, 1)):
        assert _call(lib, patches_d, counts_d, bad, _params(), out) != 0, bad
        assert lib.ubd_last_error().decode().startswith(ENTRY)
    for args in ((None, counts_d, _params(), out), (patches_d, None, _params(), out), (patches_d, counts_d, None, out), (patches_d, counts_d, _params(), None)):
        assert _call(lib, args[0], args[1], shape, args[2], args[3]) != 0
        assert lib.ubd_last_error().decode().startswith(ENTRY) and "null" in lib.ubd_last_error().decode()
    assert _call(lib, patches_d, counts_d, shape, _params(), out, offset=GUARD + 2) != 0
    assert lib.ubd_last_error().decode().startswith(ENTRY) and "aligned" in lib.ubd_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENT).all()


def test_the_older_entries_refuse_the_postal_bits(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * 4 * ROW,), SENT, dtype=torch.uint8, device="cuda")
    for entry, own in OLDER.items():
        for value in (1024, 2048, 4096, 8192, 15360, own[-1] | 1024, own[0] | 8192):
            assert _call(lib, patches_d, counts_d, mixed_patches.shape, _params(symbologies=value), out, entry=entry, offset=0) != 0, (entry, value)
            assert lib.ubd_last_error().decode().startswith(entry) and "symbologies" in lib.ubd_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENT).all()


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


def test_predict_decoded_reads_the_postal_kinds_beside_the_eight(golden_dir):
    """The frames of tests/test_gpu_extra_decode.py::test_predict_decoded_reads_all_eight_kinds and one upright frame per postal
    kind: at pixel_threshold 0.3 every pixel of the randomly initialised detector is positive and each frame is one box."""
    import extra_decode_oracle as xo
    from oracle import net_numpy as onet
    from test_gpu_extra_decode import EAN13_A, EAN8_A, UPCE_A
    from ubdvss_amd import results_to_records, text_results_to_records, width_results_to_records
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
    postal = [pc.postnet_bars("80122"), pc.planet_bars(PLANET_DIGITS), pc.rm4scc_bars(RM_TEXT), pc.kix_bars(KIX_TEXT)]
    frames += [np.repeat(pc.render(bars, 4.0, 2.0, h=120, w=320, height=0.6), 3, axis=2) for bars in postal]
    kw = dict(scan_rows=32, patch_size=(64, 384))                       # the frames' bars are 1.9 pixels wide in such a patch
    scan = dict(scan_rows=32)
    found, decoded = runner.predict_decoded(model, frames, symbologies=479 | 15360, **kw)
    assert [_key(o) for o in found] == [_key(o) for o in runner.predict_images(model, frames)]
    assert [len(o) for o in found] == [1] * 12 and [len(r) for r in decoded] == [1] * 12
    records = [r[0] for r in decoded]
    assert [type(r) for r in records] == [DecodedBarcode] * 3 + [DecodedText] * 2 + [DecodedWidth] * 3 + [DecodedPostal] * 4
    assert [r.symbology for r in records[8:]] == ["POSTNET", "PLANET", "RM4SCC", "KIX"]
    # which way up a patch lies is the extraction's choice (the long side it starts from); the framed kinds say which it took,
    # and a KIX is read as its patch lies
    turned = records[8].upside_down
    assert [r.upside_down for r in records[8:]] == [turned, turned, turned, False]
    assert [r.text for r in records[8:]] == [SHORT_ZIP, TEXTS[po.PLANET], TEXTS[po.RM4SCC], kix_half_turned(KIX_TEXT) if turned else KIX_TEXT]
    assert [r.bars for r in records[8:]] == [32, 62, 38, 44] and [r.checked for r in records[8:]] == [True, True, True, False]
    assert all(r.votes >= 2 for r in records[8:])
    # the records are the oracles' readings of the very patches predict_patches returns
    _, patches = runner.predict_patches(model, frames, patch_size=(64, 384), expand=1.25)
    for k in range(8):
        family, to_records = (("retail", results_to_records), ("text", text_results_to_records), ("width", width_results_to_records))[(k >= 3) + (k >= 5)]
        want = xo.decode_patches(family, patches[k][None], [1], 0, symbologies=479 & xo.FAMILIES[family][2], **scan)
        assert decoded[k] == to_records(want, [1])[0], k
    for k in range(8, 12):
        assert decoded[k] == postal_results_to_records(po.decode_patches(patches[k][None], [1], 0, **scan), [1])[0], k
    older = runner.predict_decoded(model, frames, symbologies=479, **kw)[1]
    assert [r[0] for r in older] == records[:8] + [None] * 4
    assert [r[0] for r in runner.predict_decoded(model, frames, symbologies=4096 | 8192, **kw)[1]] == [None] * 10 + records[10:]
    for value in (512, 16384, 479 | 15360 | 32):
        with pytest.raises(ValueError):
            runner.predict_decoded(model, frames, symbologies=value)
