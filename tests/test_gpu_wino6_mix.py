"""The Winograd layer's sample split with the residual x - h1 by a mixed-precision fma (wino6.hip MIX, split2h_6m: the default)
against the residual by two conversions and a subtraction (UBD_WINO6_SPLIT=cvt, split2h_6: the kernel of round 15): the same bits,
layer by layer and for the whole fp32 forward pass.  fma(x, 1, -h1) with h1 read as fp16 is exact in fp32, as x - f32(h1) is, and
both pieces are rounded by the same conversion, so torch.equal / np.array_equal is the check, not a tolerance.  The inputs walk the
split's ranges: fp16 normals, subnormal and zero second pieces, the clamp of the scale rule."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ubdvss_amd import NetConfig, Model, _lib

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (1, 2, 3), (3, 37, 91), (2, 72, 100))


def _under(env, make):
    """make() with UBD_WINO6_SPLIT set to env (None: unset); the switch is read when a handle is created"""
    old = os.environ.pop("UBD_WINO6_SPLIT", None)
    try:
        if env is not None: os.environ["UBD_WINO6_SPLIT"] = env
        return make()
    finally:
        os.environ.pop("UBD_WINO6_SPLIT", None)
        if old is not None: os.environ["UBD_WINO6_SPLIT"] = old


class _Layers:
    """one handle with random kernels for L4..L9 and random or zero biases, packed once"""

    def __init__(self, zero_bias):
        self.lib = _lib.load()
        self.m = Model(NetConfig(grey=False), seed=21)
        w = self.m.get_weights()
        rng = np.random.default_rng(3)
        for i in range(10, 22, 2):
            w[i] = np.zeros(24, np.float32) if zero_bias else rng.normal(0.0, 0.2, 24).astype(np.float32)
        self.m.set_weights(w)
        self.ws = torch.empty(int(self.lib.ubd_forward_workspace_bytes(self.m._h, 1, 4, 4)), dtype=torch.uint8, device="cuda")
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(self.lib.ubd_pack_weights(self.m._h, self.m.params.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.st), "pack")

    def __call__(self, k, x):
        n, hh, ww, _ = x.shape
        y = torch.full_like(x, float("nan"))
        _lib.check(self.lib.ubd_dilated_layer(self.m._h, self.m.params.data_ptr(), k, x.data_ptr(), y.data_ptr(), n, hh, ww,
                                              self.ws.data_ptr(), self.st), "dil")
        return y


@pytest.fixture(scope="module")
def forms():
    """{zero_bias: (default form, UBD_WINO6_SPLIT=cvt)}"""
    return {zb: (_under(None, lambda: _Layers(zb)), _under("cvt", lambda: _Layers(zb))) for zb in (False, True)}


def _inputs(shape):
    """name -> (n, h, w, 24) float32"""
    n, hh, ww = shape
    rng = np.random.default_rng(sum(shape))
    base = rng.random((*shape, 24), dtype=np.float32) - np.float32(0.3)          # [-0.3, 0.7]
    out = {"random": base, "x 2^-30": base * np.float32(2.0 ** -30), "x 2^30": base * np.float32(2.0 ** 30)}
    half = base.copy()
    half[:, :, :ww // 2] *= np.float32(2.0 ** -20)
    out["left half x 2^-20"] = half
    one = np.zeros_like(base)                      # the h2 pieces of the neighbours are fp16 subnormals and zeros under the large value's scale
    cy, cx = hh // 2, ww // 2
    one[0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2, :] = 1e-4
    one[0, cy, cx, 5] = 1e4
    out["1e4 among 1e-4"] = one
    out["zeros"] = np.zeros_like(base)
    out["below 2^-100"] = base * np.float32(2.0 ** -110)                         # the low clamp of the scale rule
    return out


@pytest.mark.parametrize("zero_bias", [False, True], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layers_bit_equal(forms, shape, zero_bias):
    new, old = forms[zero_bias]
    for name, x in _inputs(shape).items():
        xd = torch.from_numpy(x).cuda()
        for k in range(6):
            a, b = new(k, xd), old(k, xd)
            torch.cuda.synchronize()
            assert torch.equal(a, b), (name, k, int((a != b).sum()), float((a - b).abs().max()))
        if name == "random" and not zero_bias: assert float(a.abs().max()) > 0.05


def _passes(monkeypatch, x, cus):
    from oracle import net_numpy as onet
    w = onet.init_weights(77, 3, 0, bias_scale=0.2)
    if cus: monkeypatch.setenv("UBD_TEST_NUM_CUS", cus)
    out = []
    for env in (None, "cvt"):
        def make():
            m = Model(NetConfig(grey=False)); m.set_weights(w)
            return m
        out.append(_under(env, make).predict_on_device(torch.from_numpy(x).cuda()).cpu().numpy())
    return out


def test_pass_bit_equal_32x256(monkeypatch):
    x = np.random.default_rng(8).random((1, 32, 256, 3), dtype=np.float32) * 2 - 1
    a, b = _passes(monkeypatch, x, None)
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 1e-5
    assert np.array_equal(a, b), float(np.abs(a - b).max())


def test_pass_bit_equal_one_cu(monkeypatch):
    """three 136 x 200 images on a library that sizes its grids for ONE compute unit: many groups per wave, so the row scale is handed
    over from row to row and from group to group many times"""
    x = np.random.default_rng(9).random((3, 136, 200, 3), dtype=np.float32) * 2 - 1
    a, b = _passes(monkeypatch, x, "1")
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 1e-5
    assert np.array_equal(a, b), float(np.abs(a - b).max())
