"""GPU: ubd_decode_matrix_patches (Data Matrix ECC 200, 10 x 10 to 26 x 26) against the numpy restatement
tests/matrix_decode_oracle.py, which tests/test_matrix_decode_host.py pins on rendered symbols.  Every comparison is
np.array_equal: no tolerance.  The result buffer is pre-filled with a sentinel and carries guards at both ends: rows of slots
without an object and the guards must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import decode_cases as dc  # noqa: E402
from decode_cases import _stripes, _tint  # noqa: E402
import matrix_decode_cases as mc  # noqa: E402
import matrix_decode_oracle as mo  # noqa: E402
import postal_decode_cases as pc  # noqa: E402
from test_matrix_decode_host import ANGLES, NONE128, TEXTS, reads_as_drawn  # noqa: E402
from ubdvss_amd import _lib, NetConfig, Model, ModelRunner, DecodedMatrix, matrix_results_to_records  # noqa: E402

pytestmark = pytest.mark.gpu

ENTRY = "ubd_decode_matrix_patches"
OLDER = ("ubd_decode_patches", "ubd_decode_text_patches", "ubd_decode_width_patches", "ubd_decode_postal_patches")
GUARD, ROW, SENT = 64, 128, 0xA5
_READ = {}                                                              # (patch bytes, shape, band, window, contrast) -> the oracle's row


def _params(**kw):
    merged = dict(mo.DEFAULTS, **kw)
    return _lib.UbdDecodeParams(*[merged[k] for k, _ in _lib.UbdDecodeParams._fields_])


def _want(patches, counts, **kw):
    """mo.decode_patches(patches, counts, SENT, **kw), each distinct patch read once"""
    p = dict(mo.DEFAULTS, **kw)
    n, cap = patches.shape[:2]
    out = np.full((n, cap, ROW), SENT, np.uint8)
    for i in range(n):
        for j in range(min(int(counts[i]), cap)):
            key = (patches[i, j].tobytes(), patches[i, j].shape, p["band"], p["window"], p["contrast"])
            if key not in _READ:
                _READ[key] = mo.decode_patch(patches[i, j], band=p["band"], window=p["window"], contrast=p["contrast"])
            out[i, j] = _READ[key]
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


def _subset():
    """one member of the acceptance set per (size, pixels per module, turn), the angles in turn, and its degraded twin: 128"""
    out = []
    for n in mc.SIZES:
        sym = mc.symbol(*((TEXTS[n][0], n, TEXTS[n][1])))
        for ppm in (4, 3) if n <= 22 else (4,):
            for turns in range(4):
                angle = ANGLES[(len(out) // 2) % 5]
                for degraded in (False, True):
                    out.append((n, turns, mc.render(sym, ppm, angle=angle, turns=turns, seed=1 + len(out) % 3, **(mc.DEGRADED if degraded else {}))[:, :, 0]))
    return out


@pytest.fixture(scope="module")
def subset():
    return _subset()


def _mixed(rng):
    """eight grey 128 x 128 patches: Data Matrix symbols beside stripes, an EAN-13, an RM4SCC and noise"""
    def sym(n):
        return mc.symbol(TEXTS[n][0], n, TEXTS[n][1])
    ean = dc.flat_patch([dc.with_check([4, 0, 0, 6, 3, 8, 1, 3, 3, 3, 9, 3])], 1, 128, 128, 10)[:, :, 0]
    return [mc.render(sym(14), 4)[:, :, 0], _stripes(rng, 128, 128), ean, mc.render(sym(20), 4, angle=-1, turns=3, seed=2, **mc.DEGRADED)[:, :, 0],
            pc.render(pc.rm4scc_bars("SN34RD"), 4.0, 2.0, h=128, w=128)[:, :, 0], mc.render(sym(26), 4, angle=2, turns=2)[:, :, 0],
            rng.integers(0, 256, (128, 128), dtype=np.uint8), mc.render(sym(10), 3, turns=1)[:, :, 0]]


MIXED_READS = {0: (14, 0), 3: (20, 3), 5: (26, 2), 7: (10, 1)}          # slot -> (size, turns); every other slot reads as none


@pytest.fixture(scope="module")
def mixed_patches():
    return np.stack(_mixed(np.random.default_rng(31))).reshape(2, 4, 128, 128, 1)


@pytest.mark.parametrize("c", [1, 3])
def test_the_acceptance_subset(subset, c):
    """batched as (n, 4) with three objects an image, grey or tinted: the device reads each as the oracle does, which is as it
    was drawn, and leaves the fourth slot alone.  The tint (channel gains of 0.6..1.0, truncated) takes contrast away, and the
    set is narrowed under it where the issue lets it be, at +-2 degrees: a degraded member at +-2 degrees must equal the oracle
    but need not read (INTEGRATION.md names the class: 24 x 24, degraded, 2 degrees, the dashed side to the left)"""
    members = subset + [subset[0]] * (-len(subset) % 3)                 # a clean member fills the last image
    grey = np.zeros((len(members) // 3, 4, 128, 128), np.uint8)
    for k, m in enumerate(members):
        grey[k // 3, k % 3] = m[2]
    got = _run_and_check(_tint(grey, c, seed=7), [3] * (len(members) // 3))
    assert (got[:, 3] == SENT).all()
    for k, (n, turns, _) in enumerate(members):
        if c == 3 and k % 2 == 1 and abs(ANGLES[(k // 2) % 5]) == 2:
            continue
        assert reads_as_drawn(got[k // 3, k % 3].tolist(), n, turns), (n, turns, k, got[k // 3, k % 3, :12].tolist())


@pytest.mark.parametrize("c", [1, 3])
def test_mixed_patches(mixed_patches, c):
    """counts [4, 3]: the last slot is not written; the symbols read, stripes, linear symbols and noise are none"""
    got = _run_and_check(_tint(mixed_patches[..., 0], c, seed=5), [4, 3])
    assert (got[1, 3] == SENT).all()
    for k in range(7):
        r = got[k // 4, k % 4].tolist()
        if k in MIXED_READS:
            assert reads_as_drawn(r, *MIXED_READS[k]), (k, r[:12])
        else:
            assert r == NONE128, (k, r[:12])


def _corrupted(n, hit, seed):
    """the symbol of size n with one module flipped in each of ``hit`` codewords"""
    sym = mc.symbol(TEXTS[n][0], n, TEXTS[n][1]).copy()
    pm = mc.placement(n - 2)
    rng = np.random.default_rng(seed)
    for ch in rng.choice(sum(mc.CAPACITY[n]), hit, replace=False) + 1:
        r, c = np.argwhere(pm == 10 * ch + int(rng.integers(1, 9)))[0]
        sym[r + 1, c + 1] ^= 1
    return sym


@pytest.mark.parametrize("n", [10, 16, 26])
def test_corrupted_modules(n):
    """modules flipped on the bitmap so that 1, e / 2 and e / 2 + 1 codewords are hit: the first two read as drawn with that many
    corrected, the third is beyond the code and reads as none"""
    e = mc.CAPACITY[n][1]
    hits = (1, e // 2, e // 2 + 1)
    patches = np.stack([mc.render(_corrupted(n, hit, 40 + n), 4, turns=k) for k, hit in enumerate(hits)] + [np.zeros((128, 128, 1), np.uint8)])
    got = _run_and_check(patches.reshape(1, 4, 128, 128, 1), [3])
    for k, hit in enumerate(hits[:2]):
        r = got[0, k].tolist()
        assert reads_as_drawn(r, n, k) and r[5] == hit and r[6] == 0, (n, hit, r[:12])
    assert got[0, 2].tolist() == NONE128 and (got[0, 3] == SENT).all()


@pytest.mark.parametrize("kw", [dict(band=0, window=1, contrast=0), dict(band=2, window=64, contrast=255), dict(band=2, window=1, contrast=0),
                                dict(band=0, window=64, contrast=24), dict(band=2, window=16, contrast=24, scan_rows=32, quiet=16, min_votes=64)],
                         ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_parameter_extremes(mixed_patches, kw):
    _run_and_check(mixed_patches, [4, 4], **kw)


def test_patch_shapes():
    """32 x 32 holding a 10 x 10 symbol at 2 pixels a module, 33 x 47 with no symbol, 128 x 128 holding a 26 x 26"""
    rng = np.random.default_rng(5)
    small = np.stack([mc.render(mc.symbol("123456", 10), 2, h=32, w=32), rng.integers(0, 256, (32, 32, 1), dtype=np.uint8)])
    got = _run_and_check(_tint(small.reshape(1, 2, 32, 32), 3, seed=3), [2])
    assert reads_as_drawn(got[0, 0].tolist(), 10, 0) and got[0, 1].tolist() == NONE128
    odd = np.stack([_stripes(rng, 33, 47), rng.integers(0, 256, (33, 47), dtype=np.uint8), np.full((33, 47), 200, np.uint8),
                    mc.render(mc.symbol("123456", 10), 2, h=33, w=47)[:, :, 0]])
    got = _run_and_check(odd.reshape(2, 2, 33, 47, 1), [2, 1])
    assert got[0, 0].tolist() == NONE128 and got[0, 1].tolist() == NONE128 and got[1, 0].tolist() == NONE128 and (got[1, 1] == SENT).all()
    big = mc.render(mc.symbol(*((TEXTS[26][0], 26, TEXTS[26][1]))), 4, turns=1, angle=1, channels=3, seed=2, **mc.DEGRADED)
    assert reads_as_drawn(_run_and_check(big.reshape(1, 1, 128, 128, 3), [1])[0, 0].tolist(), 26, 1)


def test_graph_capture_equals_the_direct_call(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    params = _params()
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
    assert [int(v) for v in rows[:, :, 0].ravel()[:7]] == [68, 0, 0, 68, 0, 68, 0] and (rows[1, 3] == SENT).all()


def test_refusals_leave_the_results_untouched(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * GUARD + 2 * 4 * ROW,), SENT, dtype=torch.uint8, device="cuda")
    shape = mixed_patches.shape
    for value in (0, 1, 3, 4, 24, 32, 64, 128, 256, 479, 512, 1024, 15360, 16384, 32768 | 16384, 32768 | 1, 32768 | 15360, 65536, 65536 | 32768, -1,
                  -32768):
        assert _call(lib, patches_d, counts_d, shape, _params(symbologies=value), out) != 0, value
        assert lib.ubd_last_error().decode().startswith(ENTRY) and "symbologies" in lib.ubd_last_error().decode()
    for field, value in (("scan_rows", 0), ("scan_rows", 33), ("band", -1), ("band", 3), ("window", 0), ("window", 65), ("contrast", -1),
                         ("contrast", 256), ("quiet", -1), ("quiet", 17), ("min_votes", 0), ("min_votes", 17)):
        assert _call(lib, patches_d, counts_d, shape, _params(**{field: value}), out) != 0, (field, value)
        assert lib.ubd_last_error().decode().startswith(ENTRY) and field in lib.ubd_last_error().decode()
    for bad in ((2, 4, 128, 31, 1), (2, 4, 31, 128, 1), (2, 4, 128, 129, 1), (2, 4, 129, 128, 1), (2, 4, 128, 128, 2), (0, 4, 128, 128, 1),
                (2, 0, 128, 128, 1)):
        assert _call(lib, patches_d, counts_d, bad, _params(), out) != 0, bad
        assert lib.ubd_last_error().decode().startswith(ENTRY)
    for args in ((None, counts_d, _params(), out), (patches_d, None, _params(), out), (patches_d, counts_d, None, out), (patches_d, counts_d, _params(), None)):
        assert _call(lib, args[0], args[1], shape, args[2], args[3]) != 0
        assert lib.ubd_last_error().decode().startswith(ENTRY) and "null" in lib.ubd_last_error().decode()
    assert _call(lib, patches_d, counts_d, shape, _params(), out, offset=GUARD + 2) != 0
    assert lib.ubd_last_error().decode().startswith(ENTRY) and "aligned" in lib.ubd_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENT).all()


def test_the_older_entries_refuse_the_matrix_bit(mixed_patches):
    lib = _lib.load()
    patches_d, counts_d = torch.from_numpy(mixed_patches).cuda(), torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2 * 4 * ROW,), SENT, dtype=torch.uint8, device="cuda")
    own = {"ubd_decode_patches": 3, "ubd_decode_text_patches": 4, "ubd_decode_width_patches": 24, "ubd_decode_postal_patches": 15360}
    for entry in OLDER:
        for value in (32768, own[entry] | 32768):
            assert _call(lib, patches_d, counts_d, mixed_patches.shape, _params(symbologies=value), out, entry=entry, offset=0) != 0, (entry, value)
            assert lib.ubd_last_error().decode().startswith(entry) and "symbologies" in lib.ubd_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENT).all()


def test_predict_decoded_reads_a_data_matrix_beside_the_twelve_kinds(golden_dir):
    """The twelve frames of tests/test_gpu_postal_decode.py::test_predict_decoded_reads_the_postal_kinds_beside_the_eight and one
    frame of a Data Matrix, with patch_size=(128, 128): at pixel_threshold 0.3 every pixel of the randomly initialised detector
    is positive and each frame is one box."""
    import extra_decode_cases as xc
    import text_decode_cases as tc
    import width_decode_cases as wc
    from oracle import net_numpy as onet
    from test_gpu_extra_decode import EAN13_A, EAN8_A, UPCE_A
    from test_postal_decode_host import KIX_TEXT, PLANET_DIGITS, RM_TEXT
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
    frames.append(np.repeat(mc.render(mc.symbol(*((TEXTS[16][0], 16, TEXTS[16][1]))), 6, h=160, w=160), 3, axis=2))
    kw = dict(patch_size=(128, 128), expand=1.0)
    found, decoded = runner.predict_decoded(model, frames, symbologies=479 | 15360 | 32768, **kw)
    assert [len(o) for o in found] == [1] * 13 and [len(r) for r in decoded] == [1] * 13
    record = decoded[12][0]
    assert type(record) is DecodedMatrix and (record.symbology, record.text, record.size) == ("Data Matrix", TEXTS[16][0], 16)
    assert record.gs1 is False and record.complete is True and record.raw == b""
    # the record is the oracle's reading of the very patch predict_patches returns
    _, patches = runner.predict_patches(model, frames, **kw)
    assert patches[12].shape == (1, 128, 128, 3)
    assert decoded[12] == matrix_results_to_records(mo.decode_patches(patches[12][None], [1], 0), [1])[0]
    # masks without bit 15 give what they gave
    older = runner.predict_decoded(model, frames, symbologies=479 | 15360, **kw)[1]
    assert older[12] == [None]
    for k in range(12):
        assert decoded[k] == older[k] or (older[k] == [None] and type(decoded[k][0]) is DecodedMatrix), k
    wide = runner.predict_decoded(model, frames[:12], symbologies=479 | 15360, scan_rows=32, patch_size=(64, 384))[1]
    assert all(r[0] is not None for r in wide)                          # the twelve still read at the patch size made for them
    for value in (16384, 512, 32, 32768 | 16384, 65536):
        with pytest.raises(ValueError):
            runner.predict_decoded(model, frames, symbologies=value, **kw)
    with pytest.raises(ValueError):
        runner.predict_decoded(model, frames, symbologies=32768, patch_size=(64, 256))
