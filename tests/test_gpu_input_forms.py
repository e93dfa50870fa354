"""Every form of the input image, through every first-layer kernel, against the CPU oracles.

The first-layer kernels pick their load path from the FORM of the image, not only from its shape:
  * ``f32``         fp32 fed as it is at a 16-byte aligned base: LDS-DMA ("plain") path;
  * ``f32_off4/12`` the same fp32 values 4 / 12 bytes past a 16-byte boundary: register-staged path;
  * ``f32raw_mob``  fp32 holding the integers 0..255 with UBD_PRE_MOBILENET (reachable through the C ABI only, include/ubd.h):
                    the division branch of every kernel;
  * ``u8_mob``      uint8 with UBD_PRE_MOBILENET (lookup table / per-element conversion), also at byte offsets 1 and 3;
  * ``u8_none``     uint8 with UBD_PRE_NONE (raw pixels fed as 0..255), also at byte offset 2.
``f32raw_none`` (the fp32 integers with UBD_PRE_NONE: plain fp32 input) is the bit-identity partner of ``u8_none``.

Inputs.  The fp32 images are ``xf = (x8 - 127.5) / 127.5`` evaluated in fp32 (synthetic.noise_images), which is exactly what the
device's fused preprocessing makes of the integers x8: the oracle input of the MOBILENET forms is therefore ``xf`` in fp64, shared
with the fp32 forms, and ``u8_mob`` / ``f32raw_mob`` must give the same bits as ``f32``.  The raw-pixel forms (``u8_none`` and every
16-bit or train-step case fed raw pixels) run with L1's depthwise kernel scaled by 1/128 (a power of two: exact), which keeps
the logits out of the saturated range of the loss and the fp16 activations finite; the fp32 forms run with unscaled weights.

Gates are the suite's, not loosened: ``_check`` of test_gpu_forward.py for fp32 logits, GATE_SAME_ROUNDING / GATE_FP64 and the
binary-map margins of test_gpu_forward16.py, test_gpu_train.py's loss 1e-4 / tensor 1e-3 (relative L2) for the fp32 train step and
test_gpu_forward16._train_step_16bit_case's two gates for the 16-bit one.  Bit identities between forms that stage the same values
are asserted exactly: the forward pass has no cross-tile reductions, and the train step's grid does not depend on the input form.
Every case is run and every failure collected before the test fails, so one run is the whole report."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import net_numpy as onet, net_torch as otorch
from ubdvss_amd import NetConfig, Model, ModelRunner, Trainer, Adam, PreprocessingType, synthetic, _lib
from test_gpu_forward import _check
from test_gpu_forward16 import GATE_SAME_ROUNDING, GATE_FP64

pytestmark = pytest.mark.gpu

F32, U8 = _lib.UBD_IN_F32, _lib.UBD_IN_U8
NONE, MOB = _lib.UBD_PRE_NONE, _lib.UBD_PRE_MOBILENET
TRAIN_LOSS_TOL, TRAIN_GRAD_TOL = 1e-4, 1e-3                          # test_gpu_train.py
TRAIN16_TOL32, TRAIN16_TOL64 = 5e-3, {"bfloat16": 4e-2, "float16": 3e-2}   # test_gpu_forward16.py: test_train_step_16bit
FWD_SHAPES = ((2, 72, 100), (1, 132, 68), (3, 64, 200))              # ragged at every resolution
FWD_CLASSES = (0, 2, 1)


def offset_view(t, nbytes):
    """A contiguous copy of ``t`` inside a larger buffer of the same dtype, starting ``nbytes`` past a 16-byte boundary."""
    es = t.element_size()
    assert nbytes % es == 0
    buf = torch.empty(t.numel() + (16 + nbytes) // es + 1, dtype=t.dtype, device=t.device)
    lead = ((-buf.data_ptr()) % 16 + nbytes) // es
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


def forms(x8, for_train=False):
    """name -> (device tensor, in_dtype, preprocessing, oracle kind): "pre" = the preprocessed fp32 values xf, "raw" = the integers.
    Train-step forms: the ones the issue lists for D / E plus the aligned fp32 and raw-fp32 partners of the bit identities."""
    xf = torch.from_numpy(((x8.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)).cuda()
    xr = torch.from_numpy(x8.astype(np.float32)).cuda()
    xu = torch.from_numpy(x8).cuda()
    f = {"f32": (xf, F32, NONE, "pre"), "f32_off4": (offset_view(xf, 4), F32, NONE, "pre"),
         "f32raw_mob": (xr, F32, MOB, "pre"), "f32raw_mob_off4": (offset_view(xr, 4), F32, MOB, "pre"),
         "u8_mob": (xu, U8, MOB, "pre"), "u8_none": (xu, U8, NONE, "raw"), "f32raw_none": (xr, F32, NONE, "raw")}
    if not for_train:
        f.update({"f32_off12": (offset_view(xf, 12), F32, NONE, "pre"),
                  "u8_mob_off1": (offset_view(xu, 1), U8, MOB, "pre"), "u8_mob_off3": (offset_view(xu, 3), U8, MOB, "pre"),
                  "u8_none_off2": (offset_view(xu, 2), U8, NONE, "raw"), "f32raw_none_off4": (offset_view(xr, 4), F32, NONE, "raw")})
    return f


# groups of forms that stage the same fp32 values in the first layer: their results must be BIT-identical
IDENTITIES = (("f32", "f32_off4", "f32_off12", "u8_mob", "u8_mob_off1", "u8_mob_off3", "f32raw_mob", "f32raw_mob_off4"),
              ("u8_none", "u8_none_off2", "f32raw_none", "f32raw_none_off4"))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def abi_forward(m, x, in_dtype, pre):
    """ubd_forward with an explicit (in_dtype, preprocessing) pair on a fresh workspace (weights packed by the call)."""
    lib = _lib.load()
    n, hh, ww, _ = x.shape
    ws = torch.empty(int(lib.ubd_forward_workspace_bytes(m._h, n, hh, ww)), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, hh // 4, ww // 4, m.k_out), dtype=torch.float32, device="cuda")
    _lib.check(lib.ubd_forward(m._h, m.params.data_ptr(), x.data_ptr(), in_dtype, pre, n, hh, ww, out.data_ptr(),
                               ws.data_ptr(), ws.numel(), _stream()), "ubd_forward")
    return out.cpu().numpy()


def abi_train_step(m, x, in_dtype, pre, labels):
    """ubd_train_step with an explicit (in_dtype, preprocessing) pair: (loss[16], flat gradients) as numpy."""
    lib = _lib.load()
    n, hh, ww, _ = x.shape
    y = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    grads = torch.empty(m.params.numel(), dtype=torch.float32, device="cuda")
    loss = torch.empty(16, dtype=torch.float32, device="cuda")                      # UBD_LOSS_FLOATS
    ws = torch.empty(int(lib.ubd_train_workspace_bytes(m._h, n, hh, ww)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.ubd_train_step(m._h, m.params.data_ptr(), x.data_ptr(), in_dtype, pre, y.data_ptr(), n, hh, ww,
                                  grads.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ubd_train_step")
    return loss.cpu().numpy(), grads.cpu().numpy()


def _cfg(cin, ncls, fml, pre=PreprocessingType.NONE):
    return NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=(cin == 1), fml_compatible=fml,
                     preprocessing=pre)


def _model(cin, ncls, fml, w, dtype="float32"):
    m = Model(_cfg(cin, ncls, fml), dtype=dtype)
    m.set_weights(w)
    return m


def raw_weights(w):
    """L1's depthwise kernel scaled by 1/128 (exact) for images fed as raw pixels 0..255."""
    w = [a.copy() for a in w]
    w[0] = (w[0] * np.float32(1.0 / 128.0)).astype(np.float32)
    return w


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


_ORACLE = {}


def _oracle(key, fn):
    """oracle results shared across forms, stem variants and CU counts of the same image and weights"""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _fwd_case(cin, ncls, fml, shape, seed):
    """(uint8 image x8, {kind: weights}, {kind: fp64 oracle logits}) for the kinds "pre" and "raw" (see forms)"""
    n, hh, ww = shape
    x8 = synthetic.noise_images(seed, n, hh, ww, cin, as_float=False)
    w = onet.init_weights(700 + seed, cin, ncls, bias_scale=0.25)
    wr = raw_weights(w)
    xf = synthetic.noise_images(seed, n, hh, ww, cin)
    assert np.array_equal(xf, ((x8.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32))
    refs = {"pre": _oracle(("f64", "pre", cin, ncls, fml, shape, seed), lambda: onet.forward(xf.astype(np.float64), w, fml)),
            "raw": _oracle(("f64", "raw", cin, ncls, fml, shape, seed), lambda: onet.forward(x8.astype(np.float64), wr, fml))}
    return x8, {"pre": w, "raw": wr}, refs


def _identities(outs, what, fails):
    for group in IDENTITIES:
        have = [g for g in group if g in outs]
        for g in have[1:]:
            if not np.array_equal(outs[g], outs[have[0]]):
                d = float(np.abs(outs[g].astype(np.float64) - outs[have[0]]).max())
                fails.append(f"{what}: {g} differs from {have[0]} (max |diff| {d:.3e}): not bit-identical")


def _run_fp32_forward(cin, ncls, fml, shape, seed, fails, worst):
    x8, ws, refs = _fwd_case(cin, ncls, fml, shape, seed)
    models = {k: _model(cin, ncls, fml, w) for k, w in ws.items()}
    outs = {}
    for name, (x, dt, pre, kind) in forms(x8).items():
        what = f"cin {cin} classes {ncls} fml {fml} {shape} {name}"
        try:
            lg = abi_forward(models[kind], x, dt, pre)
        except RuntimeError as e:                                       # fml False must reach the separate kernels: no error either
            fails.append(f"{what}: {e}")
            continue
        outs[name] = lg
        ref = refs[kind]
        err = float(np.abs(lg.astype(np.float64) - ref).max())
        worst["fp32"] = max(worst["fp32"], err / (2e-5 * np.abs(ref).max() + 1e-6))
        try:
            _check(lg, ref)
        except AssertionError as e:
            fails.append(f"{what}: vs fp64 oracle: {e}")
    _identities(outs, f"cin {cin} classes {ncls} fml {fml} {shape}", fails)
    return outs


WORST = {}


def _report(key, worst):
    acc = WORST.setdefault(key, {})
    for k, v in worst.items():
        acc[k] = max(acc.get(k, 0.0), v)
    print(f"worst error as a fraction of the gate ({key}): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(acc.items())))


# ------------------------------------------------------------------------------------------------- A + B: fp32 forward
@pytest.mark.parametrize("few_cus", [False, True])
@pytest.mark.parametrize("stem", ["cold123", "fused123", "fused", "unfused"])
def test_fp32_forward_every_form_vs_oracle(monkeypatch, stem, few_cus):
    """Every form x UBD_STEM variant x grey / RGB x both padding rules x (every CU | two CUs: every block walks many strips or cold
    units) on shapes ragged at every resolution, against the fp64 oracle with _check's gate, and the bit identities of IDENTITIES
    (aligned vs offset fp32 and uint8, uint8 vs the same integers as fp32 with the same preprocessing, preprocessed fp32 vs uint8
    with the preprocessing fused).  fml_compatible=False runs the separate stem kernels whatever UBD_STEM says (cold123 / fused123
    apply to the fml padding only; "fused123" then fuses L2 -> L3)."""
    monkeypatch.setenv("UBD_STEM", stem)
    if few_cus:
        monkeypatch.setenv("UBD_TEST_NUM_CUS", "2")
    else:
        monkeypatch.delenv("UBD_TEST_NUM_CUS", raising=False)
    fails, worst = [], {"fp32": 0.0}
    for cin in (1, 3):
        for fml in (True, False):
            for k, (shape, ncls) in enumerate(zip(FWD_SHAPES, FWD_CLASSES)):
                _run_fp32_forward(cin, ncls, fml, shape, 10 * k + cin, fails, worst)
    _report("fp32 forward", worst)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("cin", [3, 1])
def test_fp32_forward_every_form_512_default_stem(monkeypatch, cin):
    """One 512 x 512 image at the default stem choice (the one-kernel stem with cold-started tiles: one image is too few strips)."""
    monkeypatch.delenv("UBD_STEM", raising=False)
    monkeypatch.delenv("UBD_TEST_NUM_CUS", raising=False)
    fails, worst = [], {"fp32": 0.0}
    _run_fp32_forward(cin, 0, True, (1, 512, 512), 90 + cin, fails, worst)
    _report("fp32 forward", worst)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ------------------------------------------------------------------------------------------------- C: 16-bit forward
@pytest.mark.parametrize("stem16", ["", "fused12", "split"])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_16bit_forward_every_form_vs_oracles(monkeypatch, dtype, stem16):
    """bf16 / fp16 forward of every form x UBD_STEM16 (one kernel | L1 -> L2 fused + L3 | three kernels) x grey / RGB: the gates and
    binary-map margin checks of test_gpu_forward16._run against the same-rounding and the fp64 oracle, and the bit identities.  The
    register-staged fp32 variants (!PLAIN) and the uint8 dword loads at odd byte offsets live here."""
    if stem16:
        monkeypatch.setenv("UBD_STEM16", stem16)
    else:
        monkeypatch.delenv("UBD_STEM16", raising=False)
    fails, worst = [], {"same_rounding": 0.0, "fp64": 0.0}
    for cin in (1, 3):
        for k, (shape, ncls, fml) in enumerate((((2, 72, 100), 0, True), ((1, 132, 68), 2, False))):
            seed = 10 * k + cin
            x8, ws, refs = _fwd_case(cin, ncls, fml, shape, seed)
            xin = {"pre": synthetic.noise_images(seed, *shape, cin).astype(np.float64), "raw": x8.astype(np.float64)}
            models = {kind: _model(cin, ncls, fml, w, dtype) for kind, w in ws.items()}
            outs = {}
            for name, (x, dt, pre, kind) in forms(x8).items():
                what = f"{dtype} UBD_STEM16={stem16!r} cin {cin} classes {ncls} fml {fml} {shape} {name}"
                lg = abi_forward(models[kind], x, dt, pre)
                outs[name] = lg
                ref = refs[kind]
                ref16 = _oracle((dtype, kind, cin, ncls, fml, shape, seed),
                                lambda: onet.forward(xin[kind], ws[kind], fml, act_dtype=dtype))
                scale = float(np.abs(ref).max())
                e16, e64 = float(np.abs(lg - ref16).max()) / scale, float(np.abs(lg - ref).max()) / scale
                worst["same_rounding"] = max(worst["same_rounding"], e16 / (GATE_SAME_ROUNDING[dtype] + 1e-5 / scale))
                worst["fp64"] = max(worst["fp64"], e64 / GATE_FP64[dtype])
                if not np.isfinite(lg).all():
                    fails.append(f"{what}: non-finite logits")
                    continue
                if e16 > GATE_SAME_ROUNDING[dtype] + 1e-5 / scale:
                    fails.append(f"{what}: vs same-rounding oracle {e16:.3e} of max|logit|")
                if e64 > GATE_FP64[dtype]:
                    fails.append(f"{what}: vs fp64 oracle {e64:.3e} of max|logit|")
                got = lg[..., 0] > 0.0
                for oname, r, gate in (("same-rounding", ref16, GATE_SAME_ROUNDING[dtype]), ("fp64", ref, GATE_FP64[dtype])):
                    decided = np.abs(r[..., 0]) > gate * scale
                    bad = int((got != (r[..., 0] > 0.0))[decided].sum())
                    if bad:
                        fails.append(f"{what}: binary map vs {oname} oracle: {bad} pixels outside the margin differ")
            _identities(outs, f"{dtype} UBD_STEM16={stem16!r} cin {cin} {shape}", fails)
    _report(f"{dtype} forward", worst)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ------------------------------------------------------------------------------------------------- D: fp32 train step
TRAIN_FORMS = ("f32", "f32_off4", "f32raw_mob", "f32raw_mob_off4", "u8_mob", "u8_none", "f32raw_none")


def _train_case(cin, ncls, shape, seed, labels=None, image_seed=None):
    """(x8, labels, weights per kind).  Without ``labels``: mostly positive maps (tests/soak_labels.py), so that the hard-negative
    term takes every negative and no near-tie at the k-th value can make kernel and oracle mine different pixels (with sparse
    rectangles, 2 x 64 x 96 grey with classes has such a tie: every form, the aligned fp32 one included, then moves every tensor by
    ~3e-3 while the loss agrees to 1e-7)."""
    import soak_labels
    n, hh, ww = shape
    if labels is None:
        labels = soak_labels.mostly_positive_maps(np.random.default_rng(seed), n, hh // 4, ww // 4, ncls)
    x8 = synthetic.textured_images(seed + 2 if image_seed is None else image_seed, labels, 4, cin)
    w = onet.init_weights(seed, cin, ncls, bias_scale=0.2)
    w[-2] = (w[-2] * 4).astype(np.float32)                                   # as test_gpu_train._setup: detection logits not all tiny
    return x8, labels, {"pre": w, "raw": raw_weights(w)}


@pytest.mark.parametrize("sepbwd", ["", "split"])
def test_fp32_train_step_every_form_vs_autograd(monkeypatch, sepbwd):
    """fp32 train step (sep_bwd_kernel UPS 1, or UBD_SEPBWD=split: UPS 0) fed u8_mob, u8_none, f32raw_mob (aligned and at +4 bytes) and
    f32_off4, grey / RGB, with and without classes: loss and every weight-gradient tensor against the fp64 autograd oracle at
    test_gpu_train.py's gates; gradients BIT-identical across the forms that stage the same values (the grid of launch_sep_bwd does
    not depend on the input form)."""
    if sepbwd:
        monkeypatch.setenv("UBD_SEPBWD", sepbwd)
    else:
        monkeypatch.delenv("UBD_SEPBWD", raising=False)
    fails, worst = [], {"loss": 0.0, "grads": 0.0}
    for cin in (1, 3):
        for ncls in (0, 2):
            shape, seed = (2, 64, 96), 40 + cin + ncls
            x8, labels, ws = _train_case(cin, ncls, shape, seed)
            xf = ((x8.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)
            xin = {"pre": xf.astype(np.float64), "raw": x8.astype(np.float64)}
            models = {kind: _model(cin, ncls, True, w) for kind, w in ws.items()}
            fs = forms(x8, for_train=True)
            outs = {}
            for name in TRAIN_FORMS:
                x, dt, pre, kind = fs[name]
                what = f"UBD_SEPBWD={sepbwd!r} cin {cin} classes {ncls} {shape} {name}"
                l4, g = abi_train_step(models[kind], x, dt, pre, labels)
                outs[name] = g
                loss_ref, _, _, grads_ref = _oracle(("train64", kind, cin, ncls, shape, seed), lambda: otorch.loss_and_grads(
                    xin[kind], labels[..., None], ws[kind], ncls > 0, True))
                le = abs(float(l4[0]) - loss_ref) / abs(loss_ref)
                worst["loss"] = max(worst["loss"], le / TRAIN_LOSS_TOL)
                if not le <= TRAIN_LOSS_TOL:
                    fails.append(f"{what}: loss {l4[0]} vs oracle {loss_ref}")
                off = 0
                for (nm, _), gr in zip(onet.weight_shapes(cin, ncls), grads_ref):
                    err = _rel(g[off:off + gr.size], gr.reshape(-1))
                    worst["grads"] = max(worst["grads"], err / TRAIN_GRAD_TOL)
                    if not err <= TRAIN_GRAD_TOL:
                        fails.append(f"{what}: gradient {nm} relative L2 error {err:.3e}")
                    off += gr.size
                assert off == g.size
            _identities(outs, f"UBD_SEPBWD={sepbwd!r} cin {cin} classes {ncls} gradients", fails)
    _report("fp32 train step", worst)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ------------------------------------------------------------------------------------------------- E: 16-bit train step
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("cin,ncls,fml,n,hh,ww", [(3, 0, True, 2, 64, 64), (1, 2, True, 2, 64, 96)])
def test_16bit_train_step_every_form_vs_autograd(dtype, cin, ncls, fml, n, hh, ww):
    """The 16-bit train step (sep12_16 / sep123_16 forward, sepbwd16.h L1 backward: its runtime copy-or-divide branch and the
    register-staged fp32 patch at an unaligned base) fed every train form, on the fixed shapes of test_train_step_16bit, against
    _train_step_16bit_case's two gates: the same-rounding autograd oracle evaluated in fp32 (5e-3 per tensor, relative L2) and in
    fp64 (4e-2 bf16 / 3e-2 fp16); loss within the same relative gates.  Gradients bit-identical across the identity groups."""
    shape = (n, hh, ww)
    x8, labels, ws = _train_case(cin, ncls, shape, 90 + cin, synthetic.rectangle_maps(91, n, hh // 4, ww // 4, n_classes=ncls), 92)   # its data
    xf = ((x8.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)
    xin = {"pre": xf, "raw": x8.astype(np.float32)}
    models = {kind: _model(cin, ncls, fml, w, dtype) for kind, w in ws.items()}
    fs = forms(x8, for_train=True)
    gdt = "bfloat16" if dtype == "bfloat16" else None
    fails, worst, outs = [], {"tol32": 0.0, "tol64": 0.0}, {}
    for name in TRAIN_FORMS:
        x, dt, pre, kind = fs[name]
        what = f"{dtype} cin {cin} classes {ncls} fml {fml} {shape} {name}"
        l4, g = abi_train_step(models[kind], x, dt, pre, labels)
        g = g.astype(np.float64)
        outs[name] = g
        if not np.isfinite(g).all():
            fails.append(f"{what}: non-finite gradients")
            continue
        for odt, tol, tname in ((torch.float32, TRAIN16_TOL32, "tol32"), (torch.float64, TRAIN16_TOL64[dtype], "tol64")):
            loss_ref, _, _, grads_ref = _oracle(("train16", dtype, str(odt), kind, cin, ncls, fml, shape), lambda: otorch.loss_and_grads(
                xin[kind], labels[..., None], ws[kind], ncls > 0, fml, dtype=odt, act_dtype=dtype, grad_dtype=gdt))
            le = abs(float(l4[0]) - loss_ref) / abs(loss_ref)
            worst[tname] = max(worst[tname], le / tol)
            if not le <= tol:
                fails.append(f"{what}: loss {l4[0]} vs {odt} oracle {loss_ref}")
            off = 0
            for (nm, _), gr in zip(onet.weight_shapes(cin, ncls), grads_ref):
                err = np.linalg.norm(g[off:off + gr.size] - gr.reshape(-1)) / max(np.linalg.norm(gr), 1e-30)
                worst[tname] = max(worst[tname], err / tol)
                if not err <= tol:
                    fails.append(f"{what}: gradient {nm} vs {odt} oracle: relative L2 error {err:.3e} > {tol}")
                off += gr.size
    _identities(outs, f"{dtype} cin {cin} classes {ncls} gradients", fails)
    _report(f"{dtype} train step", worst)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ------------------------------------------------------------------------------------------------- F: entry points
def test_entry_points_take_every_uint8_form(monkeypatch):
    """The public entry points with uint8 input: Model.predict on one image (static tensors of the graphed shape) and on a batch on a
    PreprocessingType.NONE config (raw pixels), predict_on_device(preprocessing=...) overriding the config either way,
    ModelRunner.predict's maps and class logits, and Trainer.train_on_batch's loss and gradients -- each against the oracle."""
    monkeypatch.delenv("UBD_STEM", raising=False)
    cin, ncls, fml = 3, 2, True
    x8, ws, refs = _fwd_case(cin, ncls, fml, (2, 72, 100), 3)
    m_none = Model(_cfg(cin, ncls, fml, PreprocessingType.NONE)); m_none.set_weights(ws["raw"])
    _check(m_none.predict(x8[:1]), refs["raw"][:1])                                         # one image: graphed-shape static tensors
    _check(m_none.predict(x8), refs["raw"])                                                 # a batch
    xu = torch.from_numpy(x8).cuda()
    _check(m_none.predict_on_device(xu).cpu().numpy(), refs["raw"])
    m_mobw = Model(_cfg(cin, ncls, fml, PreprocessingType.NONE)); m_mobw.set_weights(ws["pre"])
    _check(m_mobw.predict_on_device(xu, preprocessing=PreprocessingType.MOBILENET_LIKE).cpu().numpy(), refs["pre"])
    m_mob = Model(_cfg(cin, ncls, fml, PreprocessingType.MOBILENET_LIKE)); m_mob.set_weights(ws["raw"])
    _check(m_mob.predict_on_device(xu, preprocessing=PreprocessingType.NONE).cpu().numpy(), refs["raw"])
    _check(m_mob.predict(x8[1:]), onet.forward(synthetic.noise_images(3, 2, 72, 100, cin)[1:].astype(np.float64), ws["raw"], fml))
    # ModelRunner.predict: detection map = logit0 > threshold outside a 1e-3 margin, class logits within _check's gate
    runner = ModelRunner(_cfg(cin, ncls, fml, PreprocessingType.NONE))
    det, cls, _ = runner.predict(m_none, x8)
    thr = runner.logit_threshold
    ref = refs["raw"]
    far = np.abs(ref[..., 0] - thr) > 1e-3
    assert np.array_equal((det[..., 0] > 0)[far], (ref[..., 0] > thr)[far])
    err = float(np.abs(cls - ref[..., 1:]).max())
    assert err <= 2e-5 * np.abs(ref).max() + 1e-6, err
    # Trainer.train_on_batch: u8_none on a NONE config
    shape = (2, 64, 96)
    x8t, labels, wst = _train_case(cin, ncls, shape, 61)
    m_tr = Model(_cfg(cin, ncls, fml, PreprocessingType.NONE)); m_tr.set_weights(wst["raw"])
    tr = Trainer(m_tr, Adam())
    loss = tr.train_on_batch(x8t, labels[..., None])
    loss_ref, _, _, grads_ref = otorch.loss_and_grads(x8t.astype(np.float64), labels[..., None], wst["raw"], True, fml)
    assert abs(loss - loss_ref) <= TRAIN_LOSS_TOL * abs(loss_ref), (loss, loss_ref)
    g = tr.grads.cpu().numpy()                                                             # the step's gradients (Adam reads them)
    off = 0
    for (nm, _), gr in zip(onet.weight_shapes(cin, ncls), grads_ref):
        assert _rel(g[off:off + gr.size], gr.reshape(-1)) <= TRAIN_GRAD_TOL, nm
        off += gr.size


def test_informs_random_soak_vs_oracle(monkeypatch):
    """Random shapes (sides multiples of 4 from 16 to 160), grey / RGB, classes, both padding rules, every stem variant, every fp32
    forward form, against the fp64 oracle with the bit identities.  UBD_INFORMS_CASES scales it (default 6)."""
    rng = np.random.default_rng(4242)
    fails, worst = [], {"fp32": 0.0}
    for case in range(int(os.environ.get("UBD_INFORMS_CASES", "6"))):
        cin, ncls, fml = int(rng.choice([1, 3])), int(rng.choice([0, 0, 2])), bool(rng.integers(0, 2))
        shape = (int(rng.integers(1, 4)), 4 * int(rng.integers(4, 41)), 4 * int(rng.integers(4, 41)))
        stem = str(rng.choice(["fused123", "fused", "unfused", "cold123", ""]))
        if stem: monkeypatch.setenv("UBD_STEM", stem)
        else: monkeypatch.delenv("UBD_STEM", raising=False)
        if rng.integers(0, 2): monkeypatch.setenv("UBD_TEST_NUM_CUS", "2")
        else: monkeypatch.delenv("UBD_TEST_NUM_CUS", raising=False)
        n0 = len(fails)
        _run_fp32_forward(cin, ncls, fml, shape, 500 + case, fails, worst)
        fails[n0:] = [f"case {case} UBD_STEM={stem!r} CUs {os.environ.get('UBD_TEST_NUM_CUS', 'all')}: {f}" for f in fails[n0:]]
    _report("fp32 forward", worst)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])
