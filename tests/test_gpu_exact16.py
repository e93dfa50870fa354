"""The 16-bit forward pass (fwd16.hip, sep123_16.h; bf16 and fp16 storage) held to BIT equality with the same-rounding oracle on inputs
on which floating-point arithmetic is exact (tests/exact_cases.py: small integers times powers of two; every stage's sum of |terms| stays
below 2^22 quanta, which tests/test_exact_inputs_host.py asserts for every case run here).  Every assertion is an equality of fp32
logits: one unit of error in one element -- a tap one column off at a border, a weight in the wrong k-slot, an epilogue that reads the
unrounded accumulator -- fails it, also where all kernel variants share the fault.

What runs (each under both storage types):
  * chain: all ten layers non-trivial, every map size of exact_cases.CHAIN_MAPS, head in L9's epilogue (no classes) and as head16_kernel
    (2 classes), LDS-staged and direct dilated kernel (UBD_DILCONV16); one case again with UBD_TEST_NUM_CUS=1;
  * one dense dilated layer k = 0..5 between identity layers, identity 24-channel head and dense detection head, on 1 x 1, 2 x 3, the two
    smallest maps that stage layer k's dilation, 17 x 37; plus the small-output case of layer k; staged and direct kernel;
  * stem: identity layers and head behind it, so the logits are L3's stored output.  The nine (stem, input form, c_in, padding rule) rows
    of exact_cases.STEM_RUNS cover every pair of {one-kernel stem, UBD_STEM16=split, fused12} x {uint8 with PreprocessingType.NONE, float32
    at a 16-byte-aligned address, float32 one element past one} x {grey, RGB} x {fml, 'same'}: (one-kernel, u8, RGB, fml), (one-kernel,
    f32, grey, same), (one-kernel, f32 offset, RGB, same), (split, u8, grey, same), (split, f32, RGB, fml), (split, f32 offset, grey, fml),
    (fused12, u8, RGB, same), (fused12, f32, grey, fml), (fused12, f32 offset, RGB, fml); each on 1 x 1, 2 x 3, 17 x 37 and 18 x 26 maps;
  * the train step's forward (the stem stores a1 / a2, L9 stores its activation and applies the head in one epilogue): the counters of
    the returned loss vector against the counts taken from the oracle's exact logits.
The switches are read when the handle is created: one Model per (type, switches, c_in, classes, padding rule), reused across weight sets."""
import numpy as np
import pytest
import torch

import exact_cases as ec
from ubdvss_amd import NetConfig, Model

pytestmark = pytest.mark.gpu

_models = {}


def offset_view(t, nbytes):
    """A contiguous copy of ``t`` inside a larger buffer of the same dtype, starting ``nbytes`` past a 16-byte boundary."""
    es = t.element_size()
    buf = torch.empty(t.numel() + (16 + nbytes) // es + 1, dtype=t.dtype, device=t.device)
    lead = ((-buf.data_ptr()) % 16 + nbytes) // es
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


def _model(monkeypatch, dtype, c_in, n_classes, fml, dil16=None, stem16=None, num_cus=None):
    key = (dtype, c_in, n_classes, fml, dil16, stem16, num_cus)
    if key not in _models:
        for name, value in (("UBD_DILCONV16", dil16), ("UBD_STEM16", stem16), ("UBD_TEST_NUM_CUS", num_cus)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)
        cfg = NetConfig(class_names=[f"c{i}" for i in range(n_classes)] if n_classes else None, grey=(c_in == 1), fml_compatible=fml)
        _models[key] = Model(cfg, dtype=dtype, seed=0)
        if num_cus is not None:
            assert _models[key].num_cus == int(num_cus)
    return _models[key]


def _check(m, case, dtype, what, x=None):
    """predict == oracle, bit for bit; x: a device tensor in another input form of the case's images"""
    x8, xf, w = ec.build(case)
    m.set_weights(list(w))
    got = m.predict(xf.copy()) if x is None else m.predict_on_device(x).cpu().numpy()
    want = ec.reference(case, dtype)[0].astype(np.float32)
    assert got.dtype == np.float32
    assert np.array_equal(got, want), f"{case.name} {dtype} {what}: {ec.first_difference(got, want)}"


@pytest.mark.parametrize("dil16", [None, "direct"])
@pytest.mark.parametrize("n_classes", [0, 2])
@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_chain_equals_the_oracle(monkeypatch, dtype, n_classes, dil16):
    m = _model(monkeypatch, dtype, 3, n_classes, True, dil16=dil16)
    cases = ec.cases("chain", n_classes=n_classes)
    assert len(cases) == len(ec.CHAIN_MAPS)
    for case in cases:
        _check(m, case, dtype, f"UBD_DILCONV16={dil16}")


@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_chain_with_persistent_blocks_walking_several_tiles(monkeypatch, dtype):
    case = ec.BY_NAME[ec.ONE_CU_CASE]
    _check(_model(monkeypatch, dtype, 3, case.n_classes, True, num_cus="1"), case, dtype, "UBD_TEST_NUM_CUS=1")


@pytest.mark.parametrize("dil16", [None, "direct"])
@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_one_dense_layer_equals_the_oracle(monkeypatch, dtype, k, dil16):
    cases = ec.cases("dense", layer=k) + ec.cases("small", layer=k)
    assert len(cases) == 11
    for case in cases:
        _check(_model(monkeypatch, dtype, 3, case.n_classes, True, dil16=dil16), case, dtype, f"UBD_DILCONV16={dil16}")


@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_one_weight_off_by_one_quantum_on_the_device_fails_the_gate(monkeypatch, dtype):
    """The gate has teeth on the device too: with ONE entry of the dense layer's kernel raised by one quantum in the device's weights (tap
    (2, 0), input channel 5, output channel 7) the logits differ from the oracle's -- and equal, bit for bit, those of the oracle with the
    same entry raised."""
    for k in range(6):
        (case,) = ec.cases("dense", layer=k, n_classes=23, mh=17)
        m = _model(monkeypatch, dtype, 3, 23, True)
        m.set_weights(ec.weights_one_quantum_off(case, k))
        got = m.predict(ec.build(case)[1].copy())
        assert not np.array_equal(got, ec.reference(case, dtype)[0].astype(np.float32)), k
        want = ec.mutated_logits(case, dtype, k, "weight").astype(np.float32)
        assert np.array_equal(got, want), f"{case.name} {dtype}: {ec.first_difference(got, want)}"


@pytest.mark.parametrize("stem16,form,c_in,fml", ec.STEM_RUNS)
@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_stem_equals_the_oracle(monkeypatch, dtype, stem16, form, c_in, fml):
    m = _model(monkeypatch, dtype, c_in, 23, fml, stem16=stem16)
    cases = ec.cases("stem", c_in=c_in, fml=fml)
    assert len(cases) == len(ec.STEM_MAPS)
    for case in cases:
        x8, xf, _ = ec.build(case)
        if form == "u8":
            x = torch.from_numpy(x8.copy()).cuda()
        else:
            x = torch.from_numpy(xf.copy()).cuda()
            assert x.data_ptr() % 16 == 0
            if form == "f32_off4":
                x = offset_view(x, 4)
        _check(m, case, dtype, f"UBD_STEM16={stem16} {form}", x=x)


@pytest.mark.parametrize("name", ec.TRAIN_CASES)
def test_train_step_forward_counts_equal_the_oracle(monkeypatch, name):
    """bf16 train step on the integer weights: n_pos, tp, tn, fp, fn, n_pixels of the loss vector (loss[7:12], loss[13]) are counts of
    logit0 > 0 (strict) against the labels; the logits are exact, so the counts are the oracle's."""
    from ubdvss_amd import Trainer, Adam
    case = ec.BY_NAME[name]
    for name_, value in (("UBD_DILCONV16", None), ("UBD_STEM16", None), ("UBD_TEST_NUM_CUS", None)):
        monkeypatch.delenv(name_, raising=False)
    _, xf, w = ec.build(case)
    m = Model(NetConfig(grey=False), dtype="bfloat16", seed=0)
    m.set_weights(list(w))
    labels = (np.random.default_rng(case.seed).random((case.n, case.mh, case.mw)) < 0.4).astype(np.int32)
    tr = Trainer(m, Adam())
    tr.backward_on_device(torch.from_numpy(xf.copy()).cuda(), torch.from_numpy(labels).cuda())
    got = tr.loss.cpu().numpy()
    pred = ec.reference(case, "bfloat16")[0][..., 0] > 0
    pos = labels > 0
    want = {"n_pos": int(pos.sum()), "tp": int((pred & pos).sum()), "tn": int((~pred & ~pos).sum()), "fp": int((pred & ~pos).sum()),
            "fn": int((~pred & pos).sum()), "n_pixels": pos.size}
    have = dict(zip(("n_pos", "tp", "tn", "fp", "fn"), (int(v) for v in got[7:12])), n_pixels=int(got[13]))
    assert min(want["tp"], want["tn"], want["fp"], want["fn"]) > 0
    assert have == want and all(float(v) == int(v) for v in got[7:14]), (name, have, want)
