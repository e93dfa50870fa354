"""GPU: phase A of the one-kernel fp32 stem with L2's weight pieces held in registers for the phase (stem123.h WREG, the default)
against the serial schedule it replaces (UBD_STEM123_SCHED=serial: every row unit reads its six pieces in front of its MFMAs).

Only where the MFMAs' weight operands come from differs: every depthwise sum takes its taps in the same order, every pointwise product
chains the same six piece products per N tile, so the logits -- and everything a postprocess job makes of them -- are the SAME BITS:
np.array_equal, fp32.
The shapes are the smallest at which the walk can go wrong: one tile per row and one L3 row; two and three tiles per row with a ragged
last tile and the carried column; tile rows that need the 3-row and the 2-row waves with the border masks at all four edges; the
ticketed strip walk on two CUs; cold tiles at 1, 2 and 9 tiles per row; grey and RGB; the three input forms; one pipelined step whose
stem carries a postprocess job and a cold-tile tail."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import net_numpy as onet
from ubdvss_amd import NetConfig, Model, ModelRunner, PreprocessingType, synthetic, _lib

pytestmark = pytest.mark.gpu

SWITCH = "UBD_STEM123_SCHED"


def _model(sched, cfg, w):
    """a Model whose handle is created with UBD_STEM123_SCHED = sched (None: unset, the pipelined default); the switch is read once, there"""
    old = os.environ.pop(SWITCH, None)
    try:
        if sched is not None: os.environ[SWITCH] = sched
        m = Model(cfg)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None: os.environ[SWITCH] = old
    m.set_weights(w)
    return m


_W = {}


def _weights(cin):
    if cin not in _W: _W[cin] = onet.init_weights(41 + cin, cin, 0, bias_scale=0.2)
    return _W[cin]


def _both(monkeypatch, stem, cus, run, grey=False, pre=PreprocessingType.NONE):
    """run(model) under the default schedule and under the serial one, both with UBD_STEM = stem and (cus) UBD_TEST_NUM_CUS"""
    monkeypatch.setenv("UBD_STEM", stem)
    if cus is None: monkeypatch.delenv("UBD_TEST_NUM_CUS", raising=False)
    else: monkeypatch.setenv("UBD_TEST_NUM_CUS", cus)
    cfg = NetConfig(grey=grey, preprocessing=pre)
    out = []
    for sched in (None, "serial"):
        m = _model(sched, cfg, _weights(1 if grey else 3))
        if cus is not None: assert m.num_cus == int(cus)
        out.append(run(m))
    return out


def _same(a, b, what):
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 1e-6, (what, "the logits themselves")
    assert a.dtype == np.float32 and np.array_equal(a, b), (what, int((a != b).sum()), float(np.abs(a - b).max()))


# strip walk (UBD_STEM=fused123 takes it at any launch size): (n, H, W, CUs)
STRIPS = {
    "1x16x64 one tile per row": (1, 16, 64, None),
    "1x4x4 one L3 row": (1, 4, 4, None),
    "2x36x132 three tiles per row, ragged, carried column": (2, 36, 132, None),
    "1x20x260 five tiles per row, ragged": (1, 20, 260, None),
    "3x72x100 3-row and 2-row waves, masks at four edges": (3, 72, 100, None),
    "2x72x100 ticketed walk on two CUs": (2, 72, 100, "2"),
}


@pytest.mark.parametrize("name", list(STRIPS))
def test_strip_walk_bit_equal(name, monkeypatch):
    n, hh, ww, cus = STRIPS[name]
    x = synthetic.noise_images(6, n, hh, ww, 3)
    a, b = _both(monkeypatch, "fused123", cus, lambda m: m.predict(x))
    _same(a, b, name)


@pytest.mark.parametrize("ww", [64, 68, 512], ids=["1 tile per row", "2 tiles per row", "9 tiles per row"])
def test_cold_tiles_bit_equal(ww, monkeypatch):
    x = synthetic.noise_images(7, 2, 24, ww, 3)
    a, b = _both(monkeypatch, "cold123", None, lambda m: m.predict(x))
    _same(a, b, ww)


def _abi_forward(m, x, in_dtype, pre):
    """ubd_forward with an explicit (in_dtype, preprocessing) pair: fp32 pixels with the preprocessing fused are a form of the C ABI only"""
    lib = _lib.load()
    n, hh, ww, _ = x.shape
    ws = torch.empty(int(lib.ubd_forward_workspace_bytes(m._h, n, hh, ww)), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, hh // 4, ww // 4, m.k_out), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ubd_forward(m._h, m.params.data_ptr(), x.data_ptr(), in_dtype, pre, n, hh, ww, out.data_ptr(), ws.data_ptr(), ws.numel(), st),
               "ubd_forward")
    return out.cpu().numpy()


@pytest.mark.parametrize("form", ["grey fp32 as fed", "rgb fp32 as fed", "rgb fp32 preprocessed in the kernel", "rgb uint8", "grey uint8"])
def test_input_forms_bit_equal(form, monkeypatch):
    grey, u8 = form.startswith("grey"), form.endswith("uint8")
    cin = 1 if grey else 3
    x8 = synthetic.noise_images(8, 2, 36, 132, cin, as_float=False)
    if u8:
        a, b = _both(monkeypatch, "fused123", None, lambda m: m.predict(x8), grey=grey, pre=PreprocessingType.MOBILENET_LIKE)
    elif "preprocessed" in form:
        xr = torch.from_numpy(x8.astype(np.float32)).cuda()
        a, b = _both(monkeypatch, "fused123", None, lambda m: _abi_forward(m, xr, _lib.UBD_IN_F32, _lib.UBD_PRE_MOBILENET))
    else:
        xf = synthetic.noise_images(8, 2, 36, 132, cin)
        a, b = _both(monkeypatch, "fused123", None, lambda m: m.predict(xf), grey=grey)
    _same(a, b, form)


def test_pipelined_step_with_job_and_tail_bit_equal(monkeypatch):
    """one ModelRunner step in flight behind another: the second pass's stem carries the first batch's postprocess and hands its last
    strips out as cold tiles (tail_rows > 0 -- asked of the launch's own plan, on the two-CU grid where small batches have one)"""
    hh, ww, cap = 72, 100, 64
    monkeypatch.setenv("UBD_STEM", "fused123")
    monkeypatch.setenv("UBD_TEST_NUM_CUS", "2")
    probe = _model(None, NetConfig(grey=False), _weights(3))
    tail_rows = probe._lib.ubd_stem_tail_rows                                       # a diagnostic export, declared as tests/test_gpu_stem_cold_tail.py does
    tail_rows.restype, tail_rows.argtypes = ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4
    batch = next((n for n in range(1, 8) if int(tail_rows(probe._h, n, hh, ww, n)) > 0), None)
    if batch is None: pytest.skip("no batch below 8 gives this shape a cold-tile tail")
    labels = synthetic.rectangle_maps(3, batch, hh // 4, ww // 4)
    x = torch.from_numpy(synthetic.textured_images(4, labels, 4, 3).astype(np.float32) / 127.5 - 1.0).cuda()

    def run(m):
        assert int(tail_rows(m._h, batch, hh, ww, batch)) > 0
        runner = ModelRunner(NetConfig(grey=False), max_objects_per_image=cap, pipelined=True)
        first = runner.predict_on_device(m, x)                                        # no job yet
        second = runner.predict_on_device(m, x)                                       # carries the first batch's postprocess, with the tail
        runner.synchronize()
        res = []
        for logits, bmap, quads, _, counts in (first, second):
            c = counts.cpu().numpy()
            res.append((logits.cpu().numpy(), bmap.cpu().numpy(), c, [q[:k] for q, k in zip(quads.cpu().numpy(), np.minimum(c, cap))]))
        return res

    a, b = _both(monkeypatch, "fused123", "2", run)
    for k in range(2):
        _same(a[k][0], b[k][0], ("logits of step", k))
        assert np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][2], b[k][2]), ("binary map / counts of step", k)
        assert all(np.array_equal(p, q) for p, q in zip(a[k][3], b[k][3])), ("quads of step", k)
    assert np.array_equal(a[0][0], a[1][0]), "the pass with the job and the tail writes the logits of the pass without"
