"""GPU: the weight gradients of the train step against the oracle PER TAP of every 3 x 3 kernel and per output-channel column of the six
dilated layers, on the shapes of tests/dilated_tap_cases.py -- every tap of every dilation live, ragged sub-grids, and the second tile
column / row of a phase sub-grid at d = 4, 8 and 16 in dil_wgrad_kernel (8 x 16 tiles), dil_wgrad16_kernel (8 x 8 and 16 x 16) and the
staged forward kernel (16 x 16).  Inputs and their fairness conditions: tests/dilated_tap_cases.py, checked on the CPU by
tests/test_dilated_tap_inputs_host.py, which also shows which wrong gradients the per-tensor gates let through.

One train step per run through Trainer.backward_on_device; the flat tr.grads and tr.loss go through tap_figures() against the cached
reference.  Gates (none of them new, none fitted to what the kernels show):
  * float32: loss 1e-4 relative, EVERY figure <= 1e-3 against fp64 autograd (the SURVEY 8(d) gate of tests/test_gpu_train.py);
  * 16 bit: loss 1e-3; every figure <= TRAIN16_GATE_FP32_SOAK against the same-rounding oracle evaluated in fp32 and <= TRAIN16_GATE_FP64
    against the one evaluated in fp64 (tests/test_gpu_forward16.py);
  * forward logits of the same inputs: 2e-5 max|logit| + 1e-6 in float32 (_check of tests/test_gpu_forward.py), GATE_SAME_ROUNDING in
    16 bit.
Measured figures: profiles/r13_dilated_tap_errors.txt (UBD_TAP_REPORT=<file> appends one line per run)."""
import os

import numpy as np
import pytest
import torch

import dilated_tap_cases as tc
from test_gpu_forward import _check as check_forward32
from test_gpu_forward16 import GATE_SAME_ROUNDING, TRAIN16_GATE_FP32_SOAK, TRAIN16_GATE_FP64
from ubdvss_amd import Adam, Model, NetConfig, Trainer

pytestmark = pytest.mark.gpu

GATE_LOSS_FP32, GATE_GRAD_FP32, GATE_LOSS_16BIT = 1e-4, 1e-3, 1e-3

# variant -> (environment switch read when the handle is created, value)
VARIANTS = {"default": None, "one_cu": ("UBD_TEST_NUM_CUS", "1"), "dilconv_direct": ("UBD_DILCONV", "direct"), "sepbwd_split": ("UBD_SEPBWD", "split"),
            "dilbwd_split": ("UBD_DILBWD", "split"), "dilbwd_pair8": ("UBD_DILBWD", "pair8"), "dilconv16_direct": ("UBD_DILCONV16", "direct")}


def _references(case, dtype):
    """[(tag, reference, gate of the loss, gate of every other figure)]"""
    if dtype == "float32":
        return [("fp64 autograd", tc.reference(case), GATE_LOSS_FP32, GATE_GRAD_FP32)]
    return [("same rounding in fp32", tc.reference(case, dtype, "float32"), GATE_LOSS_16BIT, TRAIN16_GATE_FP32_SOAK),
            ("same rounding in fp64", tc.reference(case, dtype, "float64"), GATE_LOSS_16BIT, TRAIN16_GATE_FP64[dtype])]


def _report(case, dtype, variant, tag, figures):
    path = os.environ.get("UBD_TAP_REPORT")
    if not path:
        return
    top = {kind: max(((v, nm) for nm, v in figures.items() if tc.kind_of(nm) == kind), default=(0.0, "-")) for kind in ("loss", "tensor", "tap", "column")}
    with open(path, "a") as f:
        f.write(f"{case.name:13s} {dtype:9s} {variant:17s} vs {tag:22s} loss {top['loss'][0]:.1e}  tensor {top['tensor'][0]:.1e} {top['tensor'][1]:7s} "
                f"tap {top['tap'][0]:.1e} {top['tap'][1]:16s} column {top['column'][0]:.1e} {top['column'][1]}\n")


def _run(monkeypatch, case, dtype, variant="default", forward=False):
    if VARIANTS[variant]:
        monkeypatch.setenv(*VARIANTS[variant])
    w, x, labels = tc.inputs(case, dtype)
    cfg = NetConfig(class_names=[f"c{i}" for i in range(case.ncls)] if case.ncls else None, grey=(case.cin == 1), fml_compatible=case.fml)
    model = Model(cfg, dtype=dtype, seed=0)
    model.set_weights(w)
    if variant == "one_cu":
        assert model.num_cus == 1
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    where = f"{case.name} {dtype} {variant}"
    if forward:
        lg = model.predict_on_device(xt).cpu().numpy()
        ref = tc.reference(case, dtype)[1]                               # float32: the plain net; 16 bit: the same-rounding net, both in fp64
        assert lg.shape == ref.shape and lg.dtype == np.float32
        if dtype == "float32":
            try:
                check_forward32(lg, ref)
            except AssertionError as e:
                raise AssertionError(f"{where}: forward logits: {e}")
        else:
            err, scale = float(np.abs(lg - ref).max()), float(np.abs(ref).max())
            tol = GATE_SAME_ROUNDING[dtype] * scale + 1e-5
            assert err <= tol, f"{where}: forward logits differ by {err:.3e} (bound {tol:.3e}, max |logit| {scale:.3f})"
    tr = Trainer(model, Adam())
    tr.backward_on_device(xt, yt)
    loss, grads = float(tr.loss[0]), tr.grads.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss) and np.isfinite(grads).all(), where
    for tag, (loss_ref, _, grads_ref), gate_loss, gate in _references(case, dtype):
        figures = tc.gated(case, dtype, tc.tap_figures(case, loss, grads, loss_ref, grads_ref))
        _report(case, dtype, variant, tag, figures)
        bad = {nm: v for nm, v in figures.items() if not v <= (gate_loss if nm == "loss" else gate)}
        assert not bad, (f"{where} vs {tag}: {len(bad)} of {len(figures)} figures above the gate ({gate:g}; loss {gate_loss:g}); the worst: "
                         + ", ".join(f"{nm} {v:.3e}" for nm, v in tc.worst(bad)))


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_taps_vs_oracle(monkeypatch, case, dtype):
    """default path of every case and type; the forward logits of the same inputs as well"""
    _run(monkeypatch, case, dtype, forward=True)


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("name", ["wide260", "tall130"])
def test_taps_vs_oracle_dozens_of_items_per_block(monkeypatch, name, dtype):
    """A handle sized for ONE compute unit: the grid of dil_wgrad_kernel is 8 blocks for 256 - 512 items at d = 16, so every block walks
    dozens of items through the double-buffered LDS-DMA loop and the ragged-tile zeroing with the next item's DMA in flight."""
    _run(monkeypatch, tc.BY_NAME[name], dtype, "one_cu")


@pytest.mark.parametrize("variant", ["dilconv_direct", "sepbwd_split"])
@pytest.mark.parametrize("name", ["ragged33", "wide260"])
def test_taps_vs_oracle_fp32_switches(monkeypatch, name, variant):
    """UBD_DILCONV=direct: the implicit-GEMM data gradient; UBD_SEPBWD=split: the four-wave dil_wgrad_kernel and the split separable backward"""
    _run(monkeypatch, tc.BY_NAME[name], "float32", variant)


@pytest.mark.parametrize("variant", ["dilbwd_split", "dilbwd_pair8", "dilconv16_direct"])
@pytest.mark.parametrize("name", ["ragged33", "wide260", "block130x65"])
def test_taps_vs_oracle_bf16_switches(monkeypatch, name, variant):
    """UBD_DILBWD=split: weight gradient and data gradient as two kernels; pair8: no paired sub-grids; UBD_DILCONV16=direct: the direct
    16-bit dilated kernel instead of the staged one.  block130x65: the 16 x 16 tiles' second tile row under each of them."""
    _run(monkeypatch, tc.BY_NAME[name], "bfloat16", variant)
