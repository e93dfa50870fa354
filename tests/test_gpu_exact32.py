"""The fp32 forward pass (forward.hip: stem123.h, stem23.h, sepconv_kernel, wino6.hip, head_kernel; train.hip's forward) held to BIT equality
with the oracle on inputs on which floating-point arithmetic is exact (tests/exact_cases.py, the fp32 families; every stage's sum of |terms|
stays below 2^22 quanta and every dilated layer's Winograd-domain sums below 2^22 quarter quanta, which tests/test_exact_inputs_host.py
asserts for every case run here).  Every assertion is an equality of fp32 logits (or of integer counts taken from them): one unit of error
in one element fails it, also where all forms of a kernel share the fault -- a piece product of the stem's three-way bf16 split
(split3.h) dropped or in the wrong slot, a bias added on the wrong side of an unscale, the inherited 33rd L2 column or the last ragged tile
row one ulp off.  The host test certifies that each of the six kept piece products of L2's and of L3's pointwise stage is live in some
case and that the oracle's logits change when one is left out.

What runs:
  * stem32: identity dilated layers and identity head, so the logits ARE L3's output.  The fifteen rows of exact_cases.STEM32_RUNS cover
    every pair of {UBD_STEM unset, fused123, cold123, fused, unfused} x {uint8 with PreprocessingType.NONE, float32 at a 16-byte-aligned
    address (LDS-DMA), float32 one element past one (register-fed)} x {grey, RGB} x {fml, 'same'}, each on all seven map sizes of
    STEM32_MAPS and all six settings (the uint8 form: the five whose images fit); fused123 and cold123 again on a 2-CU grid (blocks walk
    several strips, the carried column crosses tiles and strip starts), UBD_STEM123_SCHED=serial, and one job pass with a cold tail;
  * chain32: all ten layers non-trivial on every map size of CHAIN_MAPS, head in L9's epilogue (no classes) and as head_kernel (2
    classes), under the default two-piece fp16 Winograd form, UBD_DILCONV=split3 / wino32 / direct and UBD_WINO6_LAYOUT=natural; one
    case again with UBD_TEST_NUM_CUS=1;
  * head32: a dense integer head of 1, 3 and 32 output channels behind identity layers;
  * the fp32 train step's forward: the counters of the returned loss vector against counts taken from the oracle's exact logits, under
    the default and under UBD_SEPBWD=split;
  * teeth on the device: one unit more in the third piece of one L3 pointwise weight, and in one L2 depthwise tap, in the device's
    weights: the logits differ from the oracle's and equal those of the oracle with the same entry raised, bit for bit.
The switches are read when the handle is created: one Model per (switches, c_in, classes, padding rule), reused across weight sets."""
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as ec
from ubdvss_amd import NetConfig, Model, PreprocessingType, synthetic

pytestmark = pytest.mark.gpu

SWITCHES = ("UBD_STEM", "UBD_STEM123_SCHED", "UBD_STEM_COLD_TAIL", "UBD_DILCONV", "UBD_WINO6_LAYOUT", "UBD_WINO6_SPLIT", "UBD_TEST_NUM_CUS", "UBD_SEPBWD")
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


def _model(monkeypatch, c_in, n_classes, fml, fresh=False, **switches):
    """the fp32 Model created under exactly the given switches (UBD_STEM="fused123", ...); every other switch unset"""
    key = (c_in, n_classes, fml, tuple(sorted(switches.items())))
    if fresh or key not in _models:
        assert set(switches).issubset(SWITCHES)
        for name in SWITCHES:
            if name in switches:
                monkeypatch.setenv(name, switches[name])
            else:
                monkeypatch.delenv(name, raising=False)
        cfg = NetConfig(class_names=[f"c{i}" for i in range(n_classes)] if n_classes else None, grey=(c_in == 1), fml_compatible=fml,
                        preprocessing=PreprocessingType.NONE)
        m = Model(cfg, dtype="float32", seed=0)
        if "UBD_TEST_NUM_CUS" in switches:
            assert m.num_cus == int(switches["UBD_TEST_NUM_CUS"])
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _input(case, form):
    x8, xf, _ = ec.build32(case)
    if form == "u8":
        return torch.from_numpy(x8.copy()).cuda()
    x = torch.from_numpy(xf.copy()).cuda()
    assert x.data_ptr() % 16 == 0
    return offset_view(x, 4) if form == "f32_off4" else x


def _check(m, case, what, form="f32", weights=None, want=None):
    """predict_on_device == oracle, bit for bit"""
    m.set_weights(list(ec.build32(case)[2] if weights is None else weights))
    got = m.predict_on_device(_input(case, form), preprocessing=PreprocessingType.NONE).cpu().numpy()
    want = (ec.reference32(case)[0] if want is None else want).astype(np.float32)
    assert got.dtype == np.float32
    assert np.array_equal(got, want), f"{case.name} {what} {form}: {ec.first_difference(got, want)}"
    return got


def _stem_cases(form, c_in, fml):
    cases = [c for c in ec.cases32("stem32", c_in=c_in, fml=fml) if form != "u8" or c.setting in ec.U8_SETTINGS]
    assert len(cases) == len(ec.STEM32_MAPS) * (len(ec.U8_SETTINGS) if form == "u8" else len(ec.STEM32_SETTINGS))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------- stem

@pytest.mark.parametrize("stem,form,c_in,fml", ec.STEM32_RUNS)
def test_stem_equals_the_oracle(monkeypatch, stem, form, c_in, fml):
    m = _model(monkeypatch, c_in, 23, fml, **({} if stem is None else {"UBD_STEM": stem}))
    for case in _stem_cases(form, c_in, fml):
        _check(m, case, f"UBD_STEM={stem}", form)


@pytest.mark.parametrize("form,c_in", [("u8", 3), ("f32", 1), ("f32_off4", 3)])
@pytest.mark.parametrize("stem", ["fused123", "cold123"])
def test_stem_on_two_blocks_equals_the_oracle(monkeypatch, stem, form, c_in):
    m = _model(monkeypatch, c_in, 23, True, UBD_STEM=stem, UBD_TEST_NUM_CUS="2")
    for case in _stem_cases(form, c_in, True):
        _check(m, case, f"UBD_STEM={stem} UBD_TEST_NUM_CUS=2", form)


@pytest.mark.parametrize("form,c_in,num_cus", [("u8", 1, None), ("f32", 3, "2"), ("f32_off4", 1, "2")])
def test_stem_serial_schedule_equals_the_oracle(monkeypatch, form, c_in, num_cus):
    sw = {"UBD_STEM": "fused123", "UBD_STEM123_SCHED": "serial"}
    if num_cus:
        sw["UBD_TEST_NUM_CUS"] = num_cus
    m = _model(monkeypatch, c_in, 23, True, **sw)
    for case in _stem_cases(form, c_in, True):
        _check(m, case, f"UBD_STEM123_SCHED=serial UBD_TEST_NUM_CUS={num_cus}", form)


def test_stem_job_pass_with_a_cold_tail_equals_the_oracle(monkeypatch):
    """Two job passes in a row on a 2-CU grid (as tests/test_gpu_stem_cold_tail.py::_passes drives them): the last strips are walked as
    ticketed cold tiles.  The case: the dense stem, identity layers and a dense 3-channel head.  Logits only; that a tail ran is read from
    the launch's own plan."""
    case = ec.BY_NAME32[ec.TAIL_CASE32]
    m = _model(monkeypatch, case.c_in, case.n_classes, True, fresh=True, UBD_STEM="fused123", UBD_TEST_NUM_CUS="2")
    m.set_weights(list(ec.build32(case)[2]))
    xt = _input(case, "f32")
    n, hh, ww, _ = xt.shape
    lab = synthetic.rectangle_maps(17, 3, 48, 80, n_classes=case.n_classes)   # the job's maps need not have the pass's shape
    lg = torch.from_numpy(synthetic.logits_from_maps(lab, case.n_classes, seed=18)).cuda()
    tail_rows = m._lib.ubd_stem_tail_rows                                          # a diagnostic export: declared here, as tools/_diag.py declares its own
    tail_rows.restype, tail_rows.argtypes = ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4
    rows = int(tail_rows(m._h, n, hh, ww, lg.shape[0]))
    assert rows == 8, rows                  # 10 strips of three tiles, 2 blocks own one each: room for 8; the default asks 4 per job block
    cap = 64
    outs = m.alloc_postprocess_outputs(lg.shape[0], lg.shape[1], lg.shape[2], cap)
    job = {"logits": lg, "logit_threshold": 0.0, "scale": 4, "min_area": 5, "cap": cap, "outputs": outs}
    out = torch.empty((n, hh // 4, ww // 4, 1 + case.n_classes), device="cuda")
    want = ec.reference32(case)[0].astype(np.float32)
    for k in range(2):
        out.fill_(float("nan"))                                                    # a tile nobody wrote shows
        m.predict_on_device(xt, out=out, postprocess=job)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"{case.name} job pass {k}: {ec.first_difference(got, want)}"


# ------------------------------------------------------------------------------------------------------------------------------ chain

@pytest.mark.parametrize("switches", [{}, {"UBD_DILCONV": "split3"}, {"UBD_DILCONV": "wino32"}, {"UBD_DILCONV": "direct"}, {"UBD_WINO6_LAYOUT": "natural"}],
                         ids=["default", "split3", "wino32", "direct", "natural"])
@pytest.mark.parametrize("n_classes", [0, 2])
def test_chain_equals_the_oracle(monkeypatch, n_classes, switches):
    m = _model(monkeypatch, 3, n_classes, True, **switches)
    cases = ec.cases32("chain32", n_classes=n_classes)
    assert len(cases) == len(ec.CHAIN_MAPS)
    for case in cases:
        _check(m, case, str(switches))


def test_chain_with_persistent_blocks_walking_several_tiles(monkeypatch):
    case = ec.BY_NAME32[ec.ONE_CU_CASE32]
    _check(_model(monkeypatch, 3, case.n_classes, True, UBD_TEST_NUM_CUS="1"), case, "UBD_TEST_NUM_CUS=1")


# ------------------------------------------------------------------------------------------------------------------------------- head

@pytest.mark.parametrize("n_classes", ec.HEAD32_CLASSES)
def test_head_equals_the_oracle(monkeypatch, n_classes):
    m = _model(monkeypatch, 3, n_classes, True)
    cases = ec.cases32("head32", n_classes=n_classes)
    assert len(cases) == len(ec.HEAD32_MAPS)
    for case in cases:
        got = _check(m, case, "head")
        assert got.shape[3] == 1 + n_classes


# ------------------------------------------------------------------------------------------------------------------ train-step forward

@pytest.mark.parametrize("sepbwd", [None, "split"])
@pytest.mark.parametrize("name", ec.TRAIN_CASES32)
def test_train_step_forward_counts_equal_the_oracle(monkeypatch, name, sepbwd):
    """fp32 train step on the integer weights: n_pos, tp, tn, fp, fn, n_pixels of the loss vector (loss[7:12], loss[13]) are counts of
    logit0 > 0 (strict) against the labels; the logits are exact, so the counts are the oracle's."""
    from ubdvss_amd import Trainer, Adam
    case = ec.BY_NAME32[name]
    m = _model(monkeypatch, 3, 0, True, fresh=True, **({} if sepbwd is None else {"UBD_SEPBWD": sepbwd}))
    _, xf, w = ec.build32(case)
    m.set_weights(list(w))
    labels = (np.random.default_rng(case.seed).random((case.n, case.mh, case.mw)) < 0.4).astype(np.int32)
    tr = Trainer(m, Adam())
    tr.backward_on_device(torch.from_numpy(xf.copy()).cuda(), torch.from_numpy(labels).cuda())
    got = tr.loss.cpu().numpy()
    pred = ec.reference32(case)[0][..., 0] > 0
    pos = labels > 0
    want = {"n_pos": int(pos.sum()), "tp": int((pred & pos).sum()), "tn": int((~pred & ~pos).sum()), "fp": int((pred & ~pos).sum()),
            "fn": int((~pred & pos).sum()), "n_pixels": pos.size}
    have = dict(zip(("n_pos", "tp", "tn", "fp", "fn"), (int(v) for v in got[7:12])), n_pixels=int(got[13]))
    assert min(want["tp"], want["tn"], want["fp"], want["fn"]) > 0
    assert have == want and all(float(v) == int(v) for v in got[7:14]), (name, sepbwd, have, want)


# ------------------------------------------------------------------------------------------------------------------ teeth on the device

def test_one_unit_in_the_third_piece_of_an_l3_weight_fails_the_gate(monkeypatch):
    """(1, 3) is live at L3 in this case.  With one L3 pointwise weight raised by one unit of its third piece in the device's weights the
    logits differ from the oracle's -- and equal, bit for bit, those of the oracle with the same entry raised."""
    case = ec.BY_NAME32[ec.TEETH_PW3_CASE32]
    entry, unit = ec.pw3_third_piece_entry(case)
    w = ec.weights_pw3_raised(case, entry, unit)
    m = _model(monkeypatch, case.c_in, 23, True)
    want = ec.forward32_mutated(case, None, weights=w)
    got = _check(m, case, f"L3 pointwise weight {entry} raised by {unit}", weights=w, want=want)
    assert not np.array_equal(got, ec.reference32(case)[0].astype(np.float32))


def test_one_unit_in_an_l2_depthwise_tap_fails_the_gate(monkeypatch):
    case = ec.BY_NAME32[ec.TEETH_DW2_CASE32]
    w = ec.weights_dw2_raised(case)
    m = _model(monkeypatch, case.c_in, 23, True)
    want = ec.forward32_mutated(case, "dw")
    assert np.array_equal(want, ec.forward32_mutated(case, None, weights=w))
    got = _check(m, case, "L2 depthwise tap (0, 2) of channel 11 raised by one", weights=w, want=want)
    assert not np.array_equal(got, ec.reference32(case)[0].astype(np.float32))
