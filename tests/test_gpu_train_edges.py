"""GPU: train step, forward pass, loss and class vote at the two ends of the C ABI's stated domain -- up to 31 classes (k_out = 32: the
second pair of MFMA column tiles of head_wgrad_kernel, its ragged last 64-pixel tile, the s_kT transposes, the softmax loops) and maps of
1..7 pixels per side (every dilation but 1 beyond the map, cold-tile stem only, Winograd sub-grids of one pixel or none) -- against the
fp64 oracle.  Inputs and their fairness conditions: tests/train_edge_cases.py, checked on the CPU by test_train_edge_inputs_host.py.

Gates (none of them new):
  * fp32 train step: loss 1e-4 relative, every gradient tensor 1e-3 relative L2 of fp64 autograd (tests/test_gpu_train.py);
  * 16-bit train step: TRAIN16_GATE_FP32_SOAK per tensor against the same-rounding oracle evaluated in fp32, TRAIN16_GATE_FP64 against the
    one evaluated in fp64 (tests/test_gpu_forward16.py, as its random-shape soak applies them);
  * with classes, the same number gates every one of the k_out COLUMNS of the head-kernel gradient on its own (24 values, relative L2) and
    every element of the head-bias gradient (|g - g_ref| <= gate * max|g_ref|): a wrong column does not hide behind 31 right ones;
  * a reference tensor, column or element that is exactly zero must be exactly zero on the device;
  * forward: _check of tests/test_gpu_forward.py (fp32), GATE_SAME_ROUNDING / GATE_FP64 of tests/test_gpu_forward16.py (16 bit);
  * loss alone: _check of tests/test_gpu_loss.py; class vote: _compare of tests/test_gpu_postprocess.py (bit-exact).

Worst errors observed on MI355X (a record, not a gate; printed by the module at its end, UBD_EDGE_REPORT=<file> also writes them as JSON):
                       loss     stem l1-l3  dilated l4-l9  head.k   head.b   head.k column  head.b element   gate
  float32  / fp64      8.8e-08  7.3e-06     7.1e-06        1.2e-06  7.4e-06  1.0e-05        1.1e-06          1e-4 loss, 1e-3
  bfloat16 / in fp32   1.2e-07  1.9e-03     7.9e-05        6.3e-06  6.8e-06  7.5e-06        4.4e-07          2e-2
  bfloat16 / in fp64   6.0e-08  1.9e-03     7.9e-05        4.0e-06  5.7e-06  5.3e-06        9.0e-07          4e-2
  float16  / in fp32   2.1e-06  6.2e-04     6.1e-04        4.0e-05  1.1e-05  1.3e-03        1.1e-05          2e-2
  float16  / in fp64   1.8e-06  6.4e-04     6.2e-04        2.6e-05  4.8e-06  5.5e-04        3.4e-06          3e-2
  forward, 16 bit (of max |logit|): bfloat16 2.7e-07 same rounding / 4.3e-03 fp64 (gates 2e-2 / 2.5e-2), float16 3.0e-04 / 4.7e-04
  (gates 4e-3 / 5e-3).  The fp32 forward, the loss and the class vote passed their existing checks; no kernel defect was found.
  Sensitivity, shown once on builds that are not kept: `const bool wide = false;` in head_wgrad_kernel fails exactly the k_out = 17, 24
  and 32 cases on head-kernel columns 16 and above (relative error 1.0) and passes k_out <= 16; at 2 x 40 x 36 with 16 classes the
  16-bit runs catch it ONLY through the per-column gate (the whole tensor stays inside 2e-2).
"""
import json
import os

import numpy as np
import pytest
import torch

import train_edge_cases as tc
from oracle import net_numpy as onet
from test_gpu_forward import _check as check_forward32
from test_gpu_forward16 import GATE_FP64, GATE_SAME_ROUNDING, TRAIN16_GATE_FP32_SOAK, TRAIN16_GATE_FP64
from test_gpu_loss import _check as check_loss
from test_gpu_postprocess import _compare as compare_postprocess, _model as postprocess_model
from test_stem_plan_host import SETTINGS, rules
from ubdvss_amd import Adam, Model, NetConfig, Trainer
from ubdvss_amd.net import PreprocessingType

pytestmark = pytest.mark.gpu

GATE_LOSS_FP32, GATE_GRAD_FP32 = 1e-4, 1e-3

WORST = {}                                                      # (dtype, reference, group) -> (figure, case, name)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    lines = [f"{dt:9s} vs {ref:22s} {grp:16s} {v:.2e}  ({case} {nm})" for (dt, ref, grp), (v, case, nm) in sorted(WORST.items())]
    print("\nworst observed errors:\n" + "\n".join(lines))
    path = os.environ.get("UBD_EDGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump([{"dtype": k[0], "reference": k[1], "group": k[2], "error": v[0], "case": v[1], "figure": v[2]} for k, v in sorted(WORST.items())], f, indent=1)


@pytest.fixture
def one_cu(monkeypatch):
    monkeypatch.setenv("UBD_TEST_NUM_CUS", "1")


def _config(case, u8=False):
    return NetConfig(class_names=[f"c{i}" for i in range(case.ncls)] if case.ncls else None, grey=(case.cin == 1), fml_compatible=case.fml,
                     preprocessing=PreprocessingType.MOBILENET_LIKE if u8 else PreprocessingType.NONE)


def _trainer(case, dtype):
    w, x, labels = tc.inputs(case, dtype)
    model = Model(_config(case), dtype=dtype, seed=0)
    model.set_weights(w)
    return Trainer(model, Adam()), torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()


def _gate(case, dtype, tag, loss, grads, reference, gate_loss, gate):
    """every figure of tc.errors() against its gate; all of them are looked at before the first failure is reported"""
    loss_ref, _, grads_ref = reference
    figures = tc.errors(case, loss, grads, loss_ref, grads_ref)
    bad = []
    for nm, v in figures.items():
        key = (dtype, tag, tc.group_of(nm))
        if v > WORST.get(key, (-1.0,))[0]:
            WORST[key] = (v, case.name, nm)
        if not v <= (gate_loss if nm == "loss" else gate):
            bad.append((nm, v))
    assert not bad, (case.name, dtype, tag, bad)


_RUNS = tc.train_runs()


@pytest.mark.parametrize("case,dtype", [r for r in _RUNS if not r[0].one_cu], ids=[f"{c.name}-{dt}" for c, dt in _RUNS if not c.one_cu])
def test_train_step_vs_oracle(case, dtype):
    tr, x, y = _trainer(case, dtype)
    tr.backward_on_device(x, y)
    loss, grads = float(tr.loss[0]), tr.grads.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss) and np.isfinite(grads).all()
    if dtype == "float32":
        _gate(case, dtype, "fp64 autograd", loss, grads, tc.reference(case), GATE_LOSS_FP32, GATE_GRAD_FP32)
    else:
        _gate(case, dtype, "same rounding in fp32", loss, grads, tc.reference(case, dtype, "float32"), TRAIN16_GATE_FP32_SOAK, TRAIN16_GATE_FP32_SOAK)
        _gate(case, dtype, "same rounding in fp64", loss, grads, tc.reference(case, dtype, "float64"), TRAIN16_GATE_FP64[dtype], TRAIN16_GATE_FP64[dtype])


@pytest.mark.parametrize("case", [c for c in tc.CASES if c.one_cu], ids=lambda c: c.name)
def test_train_step_vs_oracle_several_head_tiles_per_block(one_cu, case):
    """3 x 72 x 104 (1404 map pixels: 21 head tiles and one of 60) on a handle sized for ONE compute unit: a few blocks walk several
    64-pixel tiles each, so the register prefetch of the next tile and the ragged tile's ones column after full tiles are live."""
    tr, x, y = _trainer(case, "float32")
    assert tr.model.num_cus == 1
    tr.backward_on_device(x, y)
    _gate(case, "float32", "fp64 autograd", float(tr.loss[0]), tr.grads.cpu().numpy().astype(np.float64), tc.reference(case), GATE_LOSS_FP32, GATE_GRAD_FP32)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_gradients_of_31_classes_repeat_bit_for_bit(dtype):
    """The promise of test_gradients_repeat_bit_for_bit (tests/test_gpu_train.py) at k_out = 32: ragged head tiles, whole ones, a tiny map."""
    for name in ("classes31_2x40x36", "classes31_1x64x96", "tiny_3x12x20_cls31"):
        tr, x, y = _trainer(tc.BY_NAME[name], dtype if tc.BY_NAME[name].seeds[dtype] is not None else "float32")
        tr.backward_on_device(x, y)
        first, loss = tr.grads.clone(), tr.loss.clone()
        assert torch.isfinite(first).all() and float(first.abs().max()) > 0
        tr.backward_on_device(x, y)
        assert torch.equal(tr.grads, first) and torch.equal(tr.loss, loss), name


# ------------------------------------------------------------------------------------------------------------------- forward
def _check_forward16(lg, ref16, ref64, dtype):
    """the two gates of tests/test_gpu_forward16.py (_run)"""
    scale = float(np.abs(ref64).max())
    e16, e64 = float(np.abs(lg - ref16).max()) / scale, float(np.abs(lg - ref64).max()) / scale
    for tag, v in (("same rounding", e16), ("fp64", e64)):
        key = (dtype, tag, "forward logits")
        if v > WORST.get(key, (-1.0,))[0]:
            WORST[key] = (v, "", "max |diff| / max |logit|")
    assert e16 <= GATE_SAME_ROUNDING[dtype] + 1e-5 / scale, (e16, e64)
    assert e64 <= GATE_FP64[dtype], (e16, e64)


_SWEEP = [c for c in tc.CLASS_CASES if not c.one_cu and 1 + c.ncls in (16, 17, 32)]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("case", _SWEEP, ids=lambda c: c.name)
def test_forward_class_sweep(case, dtype):
    """head_kernel / head16_kernel and the head in the last layer's epilogue at k_out = 16, 17 and 32"""
    w, x, _ = tc.inputs(case, dtype)
    m = Model(_config(case), dtype=dtype)
    m.set_weights(w)
    lg = m.predict(x)
    ref = onet.forward(x.astype(np.float64), w, case.fml)
    assert lg.shape == ref.shape and lg.dtype == np.float32
    if dtype == "float32":
        check_forward32(lg, ref)
    else:
        _check_forward16(lg, onet.forward(x.astype(np.float64), w, case.fml, act_dtype=dtype), ref, dtype)


STEMS = ("", "fused123", "fused", "unfused", "cold123")


def _planned_form(stem, fml, num_cus, n, hh):
    """The form the host plan gives this model and launch (tests/test_stem_plan_host.py restates ubd_plan_stem; the handle's setting is
    the one ubd_create derives: fml models default to "fused123" unforced, others to "unfused"; "cold123" is read for fml models only)."""
    if stem == "" or (stem == "cold123" and not fml):
        setting, forced = ("fused123" if fml else "unfused"), 0
    else:
        setting, forced = stem, int(stem != "unfused")
    return rules(SETTINGS[setting], forced, int(fml), num_cus, n, hh, 1, 0)[0]


@pytest.mark.parametrize("case", tc.TINY_CASES, ids=lambda c: c.name)
def test_forward_tiny_maps_every_stem_variant(monkeypatch, case):
    """Every tiny-map case under every UBD_STEM, float and uint8 input, against the fp64 oracle.  A variant the host plan refuses or
    replaces at this size is not skipped: the plan's form is computed, the forms that must occur are asserted, and variants with the SAME
    planned form must give bit-identical logits (the replacement really ran the other form's kernels)."""
    w, x, _ = tc.inputs(case)
    x8 = tc.images_of(case, case.seeds["float32"], u8=True)
    ref = {False: onet.forward(x.astype(np.float64), w, case.fml), True: onet.forward((x8.astype(np.float64) - 127.5) / 127.5, w, case.fml)}
    out, forms = {}, {}
    for stem in STEMS:
        if stem:
            monkeypatch.setenv("UBD_STEM", stem)
        else:
            monkeypatch.delenv("UBD_STEM", raising=False)
        for u8 in (False, True):
            m = Model(_config(case, u8))
            m.set_weights(w)
            forms[stem] = _planned_form(stem, case.fml, m.num_cus, case.n, case.hh)
            lg = m.predict(x8 if u8 else x)
            try:
                check_forward32(lg, ref[u8])
            except AssertionError as e:
                raise AssertionError(f"{case.name} UBD_STEM={stem!r} ({forms[stem]}) uint8 {u8}: {e}")
            out[(stem, u8)] = lg
    if case.fml:          # a launch this small: cold tiles by default; the strip walk, L1 + stem23 and the three kernels when forced
        assert forms == {"": "cold", "fused123": "strips", "fused": "l1_stem23", "unfused": "separate", "cold123": "cold"}
    else:                 # no one-kernel stem without the fml padding: "fused123" is replaced by L1 + stem23, "cold123" is refused
        assert forms == {"": "separate", "fused123": "l1_stem23", "fused": "l1_stem23", "unfused": "separate", "cold123": "separate"}
    for a in STEMS:
        for b in STEMS:
            if a < b and forms[a] == forms[b]:
                for u8 in (False, True):
                    assert np.array_equal(out[(a, u8)], out[(b, u8)]), (case.name, a, b, forms[a], u8)


# ------------------------------------------------------------------------------------------------------------------- loss alone
@pytest.mark.parametrize("n_cls,n,h,w", [(15, 2, 16, 24), (16, 2, 16, 24), (31, 2, 16, 24), (31, 1, 1, 2)])
def test_loss_alone_many_classes(n_cls, n, h, w):
    """ubd_loss (loss_pixel's softmax loop) at 15, 16 and 31 classes, every class present; and 31 classes on two pixels"""
    rng = np.random.default_rng(100 + n_cls + h)
    yt = tc.edge_labels(200 + n_cls + h, n, h, w, n_cls, mined=False)
    assert n * h * w <= n_cls or len(np.unique(yt)) == n_cls + 1
    yp = rng.normal(0, 3.0, (n, h, w, 1 + n_cls)).astype(np.float32)
    check_loss(yt, yp, True)


# ------------------------------------------------------------------------------------------------------------------- class vote
@pytest.fixture(params=["lds", "lds_split", "global"])
def front_end(request, monkeypatch):
    """the code paths of tests/test_gpu_postprocess.py's fixture of the same name (the switches are read when a handle is created)"""
    from ubdvss_amd import _lib
    _lib.reset_static_handles()
    for k in ("UBD_PP_GLOBAL", "UBD_PP_SPLIT", "UBD_PP_SERIAL_TAIL", "UBD_PP_THREADS_512"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "global":
        monkeypatch.setenv("UBD_PP_GLOBAL", "1")
    elif request.param == "lds_split":
        monkeypatch.setenv("UBD_PP_SPLIT", "1")
    yield request.param
    _lib.reset_static_handles()


@pytest.mark.parametrize("n_cls,n,h,w,seed", tc.VOTE_CASES)
def test_class_vote_many_classes(front_end, n_cls, n, h, w, seed):
    """pp_vote_kernel's softmax loop at 16 and 31 classes, close votes (clear of ties by 1e-4: asserted on the CPU), on maps inside and
    above the one-block LDS form's 16 384 pixels: winners bit-equal to the oracle's"""
    lg = tc.vote_logits(n_cls, n, h, w, seed)
    compare_postprocess(postprocess_model(n_cls), lg, n_cls)
