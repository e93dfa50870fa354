"""One fp32 dilated layer (ubd_dilated_layer) held to BIT equality with the fp64 convolution on inputs on which its arithmetic is exact
(tests/exact_cases.py LAYER32_*: integer activations of both signs in [-64, 64), kernels -2..2 at density 0.8 times a power of two,
integer biases times the same quantum), every layer k = 0..5 on 1 x 1 x 1, 1 x 2 x 3, 3 x 37 x 91 and 2 x 72 x 100 maps.

Why every form has to be exact here (certified in tests/test_exact_inputs_host.py): F(2x2, 3x3) transforms with G in {0, +-1, +-1/2} and
B, A in {0, +-1}; transformed samples are integers of at most 9 bits and transformed kernels multiples of 1/4 quantum of at most 5 bits,
so under the power-of-two scales a kernel entry fits ONE fp16 piece (the dropped product of the two second pieces is zero) and a sample
fits two (three bf16 pieces hold 24 bits); every sum stays below 2^22 quarter quanta, so fp32 accumulation is exact in any order.  Forms:
the default two-piece fp16 form, UBD_DILCONV=split3 (three bf16 pieces), UBD_DILCONV=wino32 (fp32 MFMA) and UBD_DILCONV=direct
(implicit GEMM), each also on the inputs and biases times 2^-30 and 2^30 (the per-row sample scales at both ends), which must return the
outputs times the same power.  No form is kept on a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as ec
from ubdvss_amd import NetConfig, Model, _lib

pytestmark = pytest.mark.gpu

FORMS = (None, "split3", "wino32", "direct")


class _Layers:
    """one fp32 handle under the UBD_DILCONV setting of the moment, with the exact kernels (biases times 2^p), packed once"""

    def __init__(self, p):
        self.lib = _lib.load()
        self.m = Model(NetConfig(grey=False), seed=21)
        w = self.m.get_weights()
        lw = ec.layer32_weights()
        for k in range(6):
            w[9 + 2 * k] = lw[2 * k].astype(np.float32)
            w[10 + 2 * k] = (lw[2 * k + 1] * 2.0 ** p).astype(np.float32)
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


@pytest.mark.parametrize("p", ec.LAYER32_SCALES)
@pytest.mark.parametrize("form", FORMS)
def test_layer_equals_the_fp64_convolution(monkeypatch, form, p):
    if form is None:
        monkeypatch.delenv("UBD_DILCONV", raising=False)
    else:
        monkeypatch.setenv("UBD_DILCONV", form)
    layers = _Layers(p)
    s = 2.0 ** p
    for shape in ec.LAYER32_SHAPES:
        x = torch.from_numpy((ec.layer32_input(shape) * s).astype(np.float32)).cuda()
        for k in range(6):
            want = (ec.layer32_reference(shape, k) * s).astype(np.float32)
            got = layers(k, x).cpu().numpy()
            assert np.array_equal(got, want), f"UBD_DILCONV={form} layer {k} (dilation {ec.DIL[k]}) {shape} x 2^{p}: {ec.first_difference(got, want)}"
