"""GPU: training through the multi-scale graph (ubd_multiscale_fuse_backward, ubd_train_step_multiscale, Trainer with a
MultiscaleModel) against tests/multiscale_train_oracle.py.

The fuse adjoint is held bit for bit (its arithmetic is fixed in include/ubd.h).  The step is held at the gates of the single-scale
step, none of them new: fp32 -- loss 1e-4 relative, every weight tensor 1e-3 relative L2 of fp64 autograd (tests/test_gpu_train.py);
16 bit -- the composed oracle carries net_torch.forward's same-rounding options (act_dtype, grad_dtype) through every level, so the
gates are those of tests/test_gpu_train_edges.py: TRAIN16_GATE_FP32_SOAK against the same-rounding oracle evaluated in fp32,
TRAIN16_GATE_FP64 against the one evaluated in fp64, on every figure of train_edge_cases.errors (head columns and bias elements too).

Seeds.  The fp32 cases MINE (k = n_pos < n_neg): a case whose fp32 and fp64 evaluations pick a different k-th hard negative misses
the gates by a pixel's share of the gradient without any kernel being wrong -- a near-tie in the mined top-k, visible on the CPU
oracle as a tiny gap at rank k.  The seeds of multiscale_train_oracle.STEP_CASES keep that gap above 1e-3 relative, and the 16-bit
case takes every negative; tests/test_multiscale_train_host.py holds both on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import multiscale_train_oracle as mto  # noqa: E402
import train_edge_cases as tc  # noqa: E402
from oracle import net_numpy as onet  # noqa: E402
from test_gpu_forward16 import TRAIN16_GATE_FP32_SOAK, TRAIN16_GATE_FP64  # noqa: E402
from ubdvss_amd import Adam, Model, MultiscaleModel, NetConfig, NetManager, Trainer, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 64          # bytes on either side of a buffer under test (keeps the 16-byte alignment)
GATE_LOSS_FP32, GATE_GRAD_FP32 = 1e-4, 1e-3


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- 1. the fuse adjoint
@pytest.mark.parametrize("mh,mw,k,power", [(8, 8, 1, 3), (16, 24, 3, 2), (32, 48, 1, 1), (2, 2, 5, 1), (4, 6, 3, 1), (16, 32, 2, 4), (3, 5, 1, 0)])
@pytest.mark.parametrize("n", [1, 3])
def test_fuse_backward_is_the_fp32_oracle_bit_for_bit(mh, mw, k, power, n):
    lib = _lib.load()
    rng = np.random.default_rng(mh * 100 + mw + k * 10 + power + n)
    g = (rng.standard_normal((n, mh, mw, k)) * 10 ** rng.uniform(-3, 3, (n, mh, mw, 1))).astype(np.float32)
    want = np.concatenate([l.reshape(-1) for l in mto.fuse_backward(g, power)])
    assert want.nbytes == lib.ubd_multiscale_levels_bytes(n, mh, mw, 4 * k, 0, power)
    gt = torch.from_numpy(g).cuda()
    # 16-byte aligned output (the widest accesses the row length allows), then one that is only 4-byte aligned (the narrow form)
    for shift in (0, 4):
        out = torch.full((want.size + 2 * CANARY // 4,), 7.0, dtype=torch.float32, device="cuda")
        rc = lib.ubd_multiscale_fuse_backward(gt.data_ptr(), n, mh, mw, k, power, out.data_ptr() + CANARY + shift, _stream())
        assert rc == 0, lib.ubd_last_error()
        got = out.cpu().numpy()
        lo = (CANARY + shift) // 4
        assert (got[:lo] == 7.0).all() and (got[lo + want.size:] == 7.0).all(), "wrote outside the packed levels"
        assert np.array_equal(got[lo:lo + want.size].view(np.uint32), want.view(np.uint32)), shift
    assert np.array_equal(gt.cpu().numpy(), g)                          # dmean is only read


def test_fuse_backward_rows_cut_into_chunks():
    """a map row longer than one block's tile (4096 floats of level 0): the chunks meet without a seam, at every level"""
    lib = _lib.load()
    n, mh, mw, k, power = 1, 8, 1280, 3, 2
    g = np.random.default_rng(3).standard_normal((n, mh, mw, k)).astype(np.float32)
    want = np.concatenate([l.reshape(-1) for l in mto.fuse_backward(g, power)])
    gt = torch.from_numpy(g).cuda()
    out = torch.full((want.size + 32,), 7.0, dtype=torch.float32, device="cuda")
    assert lib.ubd_multiscale_fuse_backward(gt.data_ptr(), n, mh, mw, k, power, out.data_ptr() + 64, _stream()) == 0, lib.ubd_last_error()
    got = out.cpu().numpy()
    assert (got[:16] == 7.0).all() and (got[16 + want.size:] == 7.0).all()
    assert np.array_equal(got[16:16 + want.size].view(np.uint32), want.view(np.uint32))


def test_fuse_backward_refusals():
    lib = _lib.load()
    g = torch.zeros(4096, dtype=torch.float32, device="cuda")
    out = torch.full((8192,), 3.0, dtype=torch.float32, device="cuda")
    f = lambda *a: lib.ubd_multiscale_fuse_backward(g.data_ptr(), *a, out.data_ptr(), _stream())      # noqa: E731
    assert f(1, 12, 8, 1, 3) != 0 and b"multiples of 8" in lib.ubd_last_error()
    assert f(1, 8, 8, 1, 5) != 0 and b"outside 0..4" in lib.ubd_last_error()
    assert f(1, 8, 8, 33, 1) != 0 and b"k must be" in lib.ubd_last_error()
    assert lib.ubd_multiscale_fuse_backward(None, 1, 8, 8, 1, 1, out.data_ptr(), _stream()) != 0 and b"null" in lib.ubd_last_error()
    torch.cuda.synchronize()
    assert (out == 3.0).all()                                           # a refused call launches nothing


# ---------------------------------------------------------------------------------------------- 2. the step
def _config(cin, ncls, fml):
    return NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=(cin == 1), fml_compatible=fml)


def _trainer(cin, ncls, fml, power, w, dtype="float32", lr=None):
    model = Model(_config(cin, ncls, fml), dtype=dtype, seed=0)
    model.set_weights(w)
    ms = MultiscaleModel(model, power)
    return Trainer(ms, Adam() if lr is None else Adam(lr=lr)), ms, model


_FP32_REFERENCE = {}


def _fp32_reference(case):
    """(weights, images, labels, loss, [gradients]) of the fp64 oracle: computed once, shared, left unchanged"""
    if case not in _FP32_REFERENCE:
        cin, ncls, fml, n, hh, ww, power, seed = case
        w, x, labels = mto.step_inputs(cin, ncls, n, hh, ww, seed)
        loss, _, _, grads = mto.loss_and_grads(x, labels[..., None], w, ncls > 0, power, fml)
        _FP32_REFERENCE[case] = (w, x, labels, loss, grads)
    return _FP32_REFERENCE[case]


def _fp32_figures(cin, ncls, loss, flat, loss_ref, grads_ref):
    out, off = {"loss": abs(loss - loss_ref) / abs(loss_ref)}, 0
    for (nm, _), gr in zip(onet.weight_shapes(cin, ncls), grads_ref):
        out[nm] = tc.rel_l2(flat[off:off + gr.size], gr.reshape(-1))
        off += gr.size
    assert off == flat.size
    return out


@pytest.mark.parametrize("case", mto.STEP_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_fp32_step_vs_fp64_autograd(case):
    """(3, 2, False, 1, 32, 32, 3): the last level is a 4 x 4 image and a 1 x 1 map"""
    cin, ncls, fml, n, hh, ww, power, _ = case
    w, x, labels, loss_ref, grads_ref = _fp32_reference(case)
    tr, _, _ = _trainer(cin, ncls, fml, power, w)
    tr.backward_on_device(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda())
    figures = _fp32_figures(cin, ncls, float(tr.loss[0]), tr.grads.cpu().numpy().astype(np.float64), loss_ref, grads_ref)
    print(case, {k: f"{v:.2e}" for k, v in figures.items()})
    bad = [(nm, v) for nm, v in figures.items() if not v <= (GATE_LOSS_FP32 if nm == "loss" else GATE_GRAD_FP32)]
    assert not bad, bad


@pytest.mark.parametrize("dtype", tc.DTYPES16)
def test_16bit_step_vs_same_rounding_oracle(dtype):
    case = mto.step16_case()
    w, x, labels = tc.inputs(case, dtype)
    tr, _, _ = _trainer(case.cin, case.ncls, case.fml, mto.STEP16_POWER, w, dtype)
    tr.backward_on_device(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda())
    loss, grads = float(tr.loss[0]), tr.grads.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss) and np.isfinite(grads).all()
    for evaluated_in, gate in (("float32", TRAIN16_GATE_FP32_SOAK), ("float64", TRAIN16_GATE_FP64[dtype])):
        loss_ref, grads_ref = mto.step16_reference(dtype, evaluated_in)
        figures = tc.errors(case, loss, grads, loss_ref, grads_ref)
        worst = max(figures.items(), key=lambda kv: kv[1])
        print(dtype, "same rounding in", evaluated_in, "worst", worst, "gate", gate)
        bad = [(nm, v) for nm, v in figures.items() if not v <= gate]
        assert not bad, (evaluated_in, bad)


def test_trainer_takes_the_multiscale_graph():
    """Trainer(MultiscaleModel) gives the multi-scale gradients -- and they are NOT the single-scale gradients of the base model on
    the same batch (which is what a Trainer around a MultiscaleModel computed before the multi-scale step existed)"""
    case = (3, 0, True, 2, 64, 64, 2, 12)                               # seed 12: n_neg < n_pos, the hard-negative term takes every negative
    cin, ncls, fml, n, hh, ww, power, seed = case
    w, x, labels, loss_ref, grads_ref = _fp32_reference(case)
    assert 0 < int((labels == 0).sum()) < int((labels > 0).sum())
    tr, ms, base = _trainer(cin, ncls, fml, power, w)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    tr.backward_on_device(xt, yt)
    flat = tr.grads.cpu().numpy().astype(np.float64)
    figures = _fp32_figures(cin, ncls, float(tr.loss[0]), flat, loss_ref, grads_ref)
    bad = [(nm, v) for nm, v in figures.items() if not v <= (GATE_LOSS_FP32 if nm == "loss" else GATE_GRAD_FP32)]
    assert not bad, bad
    single = Trainer(base, Adam())
    single.backward_on_device(xt, yt)
    other = _fp32_figures(cin, ncls, float(single.loss[0]), single.grads.cpu().numpy().astype(np.float64), loss_ref, grads_ref)
    assert other["loss"] > GATE_LOSS_FP32 and min(v for nm, v in other.items() if nm != "loss") > GATE_GRAD_FP32, other
    assert tc.rel_l2(single.grads.cpu().numpy(), flat) > GATE_GRAD_FP32
    with pytest.raises(ValueError, match=r"multiples of 16 \(4 \* 2\*\*max_scale_power, max_scale_power = 2\)"):
        tr.backward_on_device(torch.zeros((1, 40, 64, 3), device="cuda"), torch.zeros((1, 10, 16), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_power_zero_is_the_single_scale_step(dtype):
    cin, ncls, fml, n, hh, ww = 3, 2, True, 2, 72, 100                   # sides that are only multiples of 4
    w, x, labels = mto.step_inputs(cin, ncls, n, hh, ww, 9)
    tr0, ms, base = _trainer(cin, ncls, fml, 0, w, dtype)
    tr1 = Trainer(base, Adam())
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    tr1.backward_on_device(xt, yt)
    tr0.backward_on_device(xt, yt)
    assert float(tr1.grads.abs().max()) > 0
    assert torch.equal(tr0.grads.view(torch.int32), tr1.grads.view(torch.int32)) and torch.equal(tr0.loss.view(torch.int32), tr1.loss.view(torch.int32))
    lib = _lib.load()
    for code in (_lib.UBD_IN_U8, _lib.UBD_IN_F32):
        assert lib.ubd_train_multiscale_workspace_bytes(base._h, code, n, hh, ww, 0) == lib.ubd_train_workspace_bytes(base._h, n, hh, ww) > 0


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])      # the types of test_gradients_repeat_bit_for_bit
def test_step_repeats_bit_for_bit(dtype):
    cin, ncls, fml, n, hh, ww, power = 1, 3, True, 2, 64, 96, 2
    w, x, labels = mto.step_inputs(cin, ncls, n, hh, ww, 22)
    tr, _, _ = _trainer(cin, ncls, fml, power, w, dtype)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    tr.backward_on_device(xt, yt)
    grads, loss = tr.grads.clone(), tr.loss.clone()
    assert torch.isfinite(grads).all() and float(grads.abs().max()) > 0
    tr.backward_on_device(xt, yt)
    assert torch.equal(tr.grads.view(torch.int32), grads.view(torch.int32)) and torch.equal(tr.loss.view(torch.int32), loss.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 3. training
def test_training_reduces_the_loss():
    cin, ncls, fml, n, hh, ww, power = 3, 0, True, 2, 64, 64, 2
    w, x, labels = mto.step_inputs(cin, ncls, n, hh, ww, 21)
    tr, _, _ = _trainer(cin, ncls, fml, power, w, lr=1e-3)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    losses = torch.stack([tr.train_step_on_device(xt, yt)[0].clone() for _ in range(20)]).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert tr.iterations == 20


def test_fit_and_save(tmp_path):
    """NetManager.build_multiscale_model -> Trainer.fit with validation -> save_model / save_inference: finite logs of ONE model, the
    multi-scale prediction follows the new weights (its packed fragments are invalidated), the files are the base net's"""
    cfg = _config(3, 0, True)
    manager = NetManager(str(tmp_path), cfg)
    manager.build_multiscale_model(max_scale_power=2, seed=1)
    ms = manager.get_model()
    w, x, labels = mto.step_inputs(3, 0, 2, 64, 64, 21)
    ms.set_weights(w)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    before = ms.predict_on_device(xt).clone()
    assert torch.equal(ms.predict_on_device(xt), before)                # the second call reuses the packed fragments

    def batches():
        while True:
            yield xt, yt
    history = Trainer(ms, Adam(lr=1e-3)).fit(batches(), steps_per_epoch=2, epochs=2, validation_data=batches(), validation_steps=1)
    assert len(history.history["loss"]) == 2
    assert np.isfinite(history.history["loss"]).all() and np.isfinite(history.history["val_loss"]).all()
    after = ms.predict_on_device(xt)
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    # the validation loss is the training loss's model: a test-mode step on the training batch equals the next train step's loss
    tr = Trainer(ms, Adam())
    val = float(tr.test_step_on_device(xt, yt)[0])
    tr.backward_on_device(xt, yt)
    assert abs(val - float(tr.loss[0])) <= 1e-4 * abs(val)
    manager.save_model(step=1)
    manager.save_inference()
    assert sorted(os.listdir(tmp_path)) == sorted(["model001.h5", "model.h5", "model_weights.h5", "inference_model.h5", "config.pkl"])
    loaded = NetManager(str(tmp_path))
    loaded.load_model()
    assert isinstance(loaded.get_model(), Model)                        # the base net's file: wrapped again by the caller
    for a, b in zip(loaded.get_model().get_weights(), ms.get_weights()):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_step_refusals_name_the_rule():
    lib = _lib.load()
    base = Model(_config(3, 0, True), seed=0)
    n, hh, ww = 1, 64, 64
    x = torch.zeros((n * hh * ww * 3 + 4,), device="cuda")
    y = torch.zeros((n, hh // 4, ww // 4), dtype=torch.int32, device="cuda")
    grads = torch.full((base.count_params(),), 3.0, device="cuda")
    loss = torch.full((16,), 3.0, device="cuda")
    need = lib.ubd_train_multiscale_workspace_bytes(base._h, _lib.UBD_IN_F32, n, hh, ww, 3)
    assert need > lib.ubd_train_workspace_bytes(base._h, n, hh, ww)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(h, w_, power, nbytes, shift=0):
        return lib.ubd_train_step_multiscale(base._h, base.params.data_ptr(), x.data_ptr() + shift, _lib.UBD_IN_F32, _lib.UBD_PRE_NONE, y.data_ptr(),
                                             n, h, w_, power, grads.data_ptr(), loss.data_ptr(), ws.data_ptr(), nbytes, _stream())
    assert call(40, 64, 3, need) != 0 and b"multiples of 32" in lib.ubd_last_error()
    assert call(64, 64, 3, need, shift=4) != 0 and b"16-byte aligned" in lib.ubd_last_error()
    assert call(64, 64, 3, need - 1) != 0 and b"workspace too small" in lib.ubd_last_error()
    assert call(64, 64, 5, need) != 0 and b"outside 0..4" in lib.ubd_last_error()
    assert lib.ubd_train_multiscale_workspace_bytes(base._h, _lib.UBD_IN_F32, n, 40, 64, 3) == 0
    assert lib.ubd_train_multiscale_workspace_bytes(base._h, _lib.UBD_IN_F32, n, 64, 64, 5) == 0
    torch.cuda.synchronize()
    assert (grads == 3.0).all() and (loss == 3.0).all()                 # a refused call launches nothing
    assert call(64, 64, 3, need) == 0, lib.ubd_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(grads).all() and torch.isfinite(loss).all() and not (grads == 3.0).all()
