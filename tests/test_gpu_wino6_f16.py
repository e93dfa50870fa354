"""The Winograd layer's default products: two fp16 pieces per value under power-of-two scales, three MFMAs per product (wino6.hip,
split2h.h).  Every test drives ubd_dilated_layer, every one of the six layers, against an fp64 direct convolution on the host, the
three-piece bf16 form (UBD_DILCONV=split3) or the layer itself on scaled inputs.

Tolerance: 1e-6 of the layer's largest output.  The simulated error of the two-piece form is 2.1e-7 (tools/sim_f16_split.py), the
fp32 accumulation of the 9 x 24 products and of the transforms carries the rest; the gate is a quarter of the 4e-6 that the
existing comparison of the split-product form with the fp32-MFMA form allows."""
import ctypes

import numpy as np
import pytest
import torch

from ubdvss_amd import NetConfig, Model, _lib

pytestmark = pytest.mark.gpu

DIL = (1, 2, 4, 8, 16, 1)
GATE = 1e-6


def _weights(zero_bias):
    """random kernels of L4..L9 (the model's initialisation) with non-zero or zero biases"""
    m = Model(NetConfig(grey=False), seed=21)
    w = m.get_weights()
    rng = np.random.default_rng(3)
    for i in range(10, 22, 2):
        w[i] = np.zeros(24, np.float32) if zero_bias else rng.normal(0.0, 0.2, 24).astype(np.float32)
    return w


class _Layers:
    """one handle under the UBD_DILCONV setting of the moment, packed once"""

    def __init__(self, w):
        self.lib = _lib.load()
        self.m = Model(NetConfig(grey=False), seed=21)
        self.m.set_weights(w)
        self.ws = torch.empty(int(self.lib.ubd_forward_workspace_bytes(self.m._h, 1, 4, 4)), dtype=torch.uint8, device="cuda")
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(self.lib.ubd_pack_weights(self.m._h, self.m.params.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.st), "pack")

    def __call__(self, k, x):
        x = x.contiguous()
        n, hh, ww, _ = x.shape
        y = torch.full_like(x, float("nan"))
        _lib.check(self.lib.ubd_dilated_layer(self.m._h, self.m.params.data_ptr(), k, x.data_ptr(), y.data_ptr(), n, hh, ww,
                                              self.ws.data_ptr(), self.st), "dil")
        torch.cuda.synchronize()
        return y


def _ref64(w, k, x):
    """relu(conv + bias) of layer k in fp64 on the host; x: numpy (n, h, w, 24) float32"""
    wk = torch.from_numpy(np.asarray(w[9 + 2 * k], np.float64)).permute(3, 2, 0, 1).contiguous()
    bk = torch.from_numpy(np.asarray(w[10 + 2 * k], np.float64))
    xi = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xi, wk, bk, padding=DIL[k], dilation=DIL[k])
    return torch.relu(y).permute(0, 2, 3, 1).numpy()


@pytest.fixture(scope="module")
def biased():
    w = _weights(False)
    return w, _Layers(w)


@pytest.fixture(scope="module")
def unbiased():
    w = _weights(True)
    return w, _Layers(w)


SHAPES = ((2, 72, 100), (3, 37, 91), (1, 1, 1), (1, 2, 3))
_inputs = {}


def _input(shape):
    if shape not in _inputs:
        rng = np.random.default_rng(sum(shape))
        _inputs[shape] = rng.random((*shape, 24), dtype=np.float32) - np.float32(0.3)
    return _inputs[shape]


def _errors(w, layers, x):
    """per layer (max |y - ref|, max |ref|) against fp64"""
    xd = torch.from_numpy(x).cuda()
    out = []
    for k in range(6):
        ref = _ref64(w, k, x)
        y = layers(k, xd).cpu().numpy().astype(np.float64)
        assert np.isfinite(y).all(), k
        out.append((float(np.abs(y - ref).max()), float(np.abs(ref).max())))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_accuracy_against_fp64(biased, shape):
    w, layers = biased
    for k, (err, top) in enumerate(_errors(w, layers, _input(shape))):
        print(f"shape {shape} layer {k} d {DIL[k]}: err / max|y| = {err / top:.3e}")
        assert top > 0.05 and err <= GATE * top, (shape, k, err / top)


def test_exact_power_of_two_scaling_and_determinism(unbiased):
    _, layers = unbiased
    x = torch.from_numpy(_input((3, 37, 91))).cuda()
    for k in range(6):
        y1 = layers(k, x)
        assert float(y1.abs().max()) > 0.1
        assert torch.equal(layers(k, x), y1)
        for p in (-30, -2, 1, 30):
            s = float(2.0 ** p)
            assert torch.equal(layers(k, x * s), y1 * s), (k, p)


def test_range_inside_a_batch(unbiased):
    """image 0 scaled by 2^-30 beside an unscaled image 1: each output is the (scaled) output of the image run alone, bit for bit"""
    _, layers = unbiased
    x = torch.from_numpy(_input((2, 72, 100))).cuda()
    s = float(2.0 ** -30)
    both = torch.cat([x[0:1] * s, x[1:2]])
    for k in range(6):
        y = layers(k, both)
        assert torch.equal(y[0:1], layers(k, x[0:1]) * s), k
        assert torch.equal(y[1:2], layers(k, x[1:2])), k


def test_range_inside_a_map(unbiased):
    """left half scaled by 2^-20: the whole map within the gate of its largest value, and the small half, 3 d + 2 columns or more away
    from the seam, within the gate of ITS OWN largest value (zero biases, or the bias would be that value)"""
    w, layers = unbiased
    hh, ww, seam = 40, 144, 72
    x = np.random.default_rng(11).random((1, hh, ww, 24), dtype=np.float32) - np.float32(0.3)
    x[:, :, :seam] *= np.float32(2.0 ** -20)
    xd = torch.from_numpy(x).cuda()
    for k in range(6):
        ref = _ref64(w, k, x)
        y = layers(k, xd).cpu().numpy().astype(np.float64)
        assert np.abs(y - ref).max() <= GATE * np.abs(ref).max(), k
        far = seam - (3 * DIL[k] + 2)
        assert far >= 16
        top = np.abs(ref[:, :, :far]).max()
        err = np.abs(y - ref)[:, :, :far].max()
        print(f"layer {k} d {DIL[k]}: small half err / its max = {err / top:.3e}")
        assert top > 0 and err <= GATE * top, (k, err / top)


def test_one_large_value_among_tiny_ones(biased):
    """a map of zeros but for one value of 1e4 whose neighbours are 1e-4: finite, and within the gate"""
    w, layers = biased
    x = np.zeros((1, 8, 64, 24), np.float32)
    x[0, 3:6, 9:12, :] = 1e-4
    x[0, 4, 10, 5] = 1e4
    for k, (err, top) in enumerate(_errors(w, layers, x)):
        assert err <= GATE * top, (k, err / top)


def test_zero_input_gives_exactly_the_bias(biased):
    w, layers = biased
    x = torch.zeros((2, 37, 91, 24), device="cuda")
    for k in range(6):
        want = torch.from_numpy(np.maximum(w[10 + 2 * k], 0.0)).cuda()
        assert bool((layers(k, x).reshape(-1, 24) == want).all()), k


@pytest.mark.parametrize("band", [8, 16])
def test_scale_does_not_depend_on_the_grouping(monkeypatch, band):
    """The full model on a 32 x 256 image (an 8 x 64 map) whose first `band` pixel columns -- the first tile column of dilation 1 (2) --
    are scaled by 2^10: the phase-major pass groups other tiles into a wave than the natural pass (UBD_WINO6_LAYOUT=natural) does, so a
    scale taken over the group instead of the tile would change bits."""
    from oracle import net_numpy as onet
    w = onet.init_weights(77, 3, 0, bias_scale=0.2)
    cfg = NetConfig(grey=False)
    monkeypatch.setenv("UBD_WINO6_LAYOUT", "natural")
    nat = Model(cfg); nat.set_weights(w)
    monkeypatch.delenv("UBD_WINO6_LAYOUT")
    ph = Model(cfg); ph.set_weights(w)
    x = np.random.default_rng(band).random((1, 32, 256, 3), dtype=np.float32) * 2 - 1
    x[:, :, :band] *= np.float32(1024.0)
    xd = torch.from_numpy(x).cuda()
    a, b = ph.predict_on_device(xd).cpu().numpy(), nat.predict_on_device(xd).cpu().numpy()
    assert float(np.abs(b).max()) > 1e-5
    assert np.array_equal(a, b), float(np.abs(a - b).max())


def test_three_piece_form_still_passes_and_agrees(monkeypatch, biased):
    w, layers = biased
    monkeypatch.setenv("UBD_DILCONV", "split3")
    old = _Layers(w)
    monkeypatch.delenv("UBD_DILCONV")
    x = _input((2, 72, 100))
    xd = torch.from_numpy(x).cuda()
    for k, (err, top) in enumerate(_errors(w, old, x)):
        assert err <= GATE * top, (k, err / top)
        d = float((old(k, xd) - layers(k, xd)).abs().max())
        assert d <= GATE * top, (k, d / top)
