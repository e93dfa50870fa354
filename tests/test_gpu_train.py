"""GPU parity of the train step (forward -> loss -> backward -> Adam) vs the fp64 torch-autograd
oracle.  Tolerances (fp32 kernels with fp32 atomics vs fp64): loss relative 1e-4; every weight
gradient tensor relative L2 error <= 1e-3 (SURVEY 8(d) gate; observed ~1e-5); parameters after the
Adam step within 1e-6 of the oracle update applied to the oracle gradients."""
import numpy as np
import pytest
import torch

from oracle import net_numpy as onet, net_torch as otorch
from ubdvss_amd import NetConfig, Model, Trainer, Adam, synthetic

pytestmark = pytest.mark.gpu


def _setup(cin, ncls, fml, n, hh, ww, seed, labels=None):
    cfg = NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=(cin == 1), fml_compatible=fml)
    model = Model(cfg, seed=0)
    w = onet.init_weights(seed, cin, ncls, bias_scale=0.2)
    # larger head so that the detection logits are not all tiny
    w[-2] = (w[-2] * 4).astype(np.float32)
    model.set_weights(w)
    if labels is None:
        labels = synthetic.rectangle_maps(seed + 1, n, hh // 4, ww // 4, n_classes=ncls)
    x = synthetic.textured_images(seed + 2, labels, 4, cin).astype(np.float32) / 127.5 - 1.0
    return model, w, x, labels


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("cin,ncls,fml,n,hh,ww", [(3, 0, True, 2, 64, 64), (1, 3, True, 2, 64, 96), (3, 2, False, 1, 128, 64), (3, 0, True, 3, 72, 104)])
def test_gradients_vs_autograd(cin, ncls, fml, n, hh, ww, labels=None, per_tap=False):
    model, w, x, labels = _setup(cin, ncls, fml, n, hh, ww, 7 + cin + ncls, labels)
    tr = Trainer(model, Adam())
    tr.backward_on_device(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda())
    loss_ref, _, _, grads_ref = otorch.loss_and_grads(x, labels[..., None], w, ncls > 0, fml)
    l4 = tr.loss.cpu().numpy()
    assert abs(l4[0] - loss_ref) <= 1e-4 * abs(loss_ref), (l4, loss_ref)
    g = tr.grads.cpu().numpy()
    off = 0
    names = [nm for nm, _ in onet.weight_shapes(cin, ncls)]
    for nm, gr in zip(names, grads_ref):
        k = gr.size
        err = _rel(g[off:off + k], gr.reshape(-1))
        assert err <= 1e-3, (nm, err)
        off += k
    assert off == g.size
    if per_tap:      # every tap of every 3 x 3 kernel and every output-channel column of l4.k .. l9.k that exists at this shape, on its own
        import dilated_tap_cases as taps
        figures = taps.tap_figures(taps.Case("soak", cin, ncls, fml, n, hh, ww), l4[0], g.astype(np.float64), loss_ref, grads_ref, live_only=True)
        bad = {nm: v for nm, v in figures.items() if nm != "loss" and not v <= 1e-3}
        assert not bad, taps.worst(bad)


def test_gradients_random_shape_soak():
    """fp32 train step on random small shapes (sides multiples of 4 from 32 to 128, 1-3 images, grey / RGB, with / without classes, both
    padding rules) against the fp64 autograd oracle, same gates as above, and the same 1e-3 on every tap and output-channel column whose
    reference is not zero (tests/dilated_tap_cases.py).  UBD_TRAIN_SOAK_CASES scales it (default 4)."""
    import os
    import soak_labels
    rng = np.random.default_rng(123)
    for case in range(int(os.environ.get("UBD_TRAIN_SOAK_CASES", "4"))):
        cin, ncls, fml = int(rng.choice([1, 3])), int(rng.choice([0, 0, 2])), bool(rng.integers(0, 2))
        top = int(os.environ.get("UBD_TRAIN_SOAK_MAXSIDE", "128")) // 4 + 1        # bigger runs: maps wider than the 16-pixel tiles at every dilation
        n, hh, ww = int(rng.integers(1, 4)), 4 * int(rng.integers(8, top)), 4 * int(rng.integers(8, top))
        if top > 64 and case % 4 == 3: ww = 512                                     # ... and the 128-wide maps of the BASELINE shapes
        # big maps: labels with k = n_neg (tests/soak_labels.py): thousands of negatives make near-ties at the k-th value likely even in fp32
        lab = soak_labels.mostly_positive_maps(rng, n, hh // 4, ww // 4, ncls) if top > 33 else None
        try:
            test_gradients_vs_autograd(cin, ncls, fml, n, hh, ww, lab, per_tap=True)
        except AssertionError as e:
            raise AssertionError(f"case {case}: cin {cin} classes {ncls} fml {fml} {n} x {hh} x {ww}: {e}")


def test_gradients_direct_dilated_kernel_path(monkeypatch):
    """fp32 train step with UBD_DILCONV=direct: forward and data gradient of the dilated layers on the implicit-GEMM kernel."""
    monkeypatch.setenv("UBD_DILCONV", "direct")
    test_gradients_vs_autograd(3, 2, True, 2, 64, 96)


@pytest.mark.parametrize("cin,ncls,n,hh,ww", [(3, 0, 3, 72, 104), (1, 3, 2, 64, 96), (3, 2, 5, 136, 200)])
def test_fp32_fused_separable_backward_vs_split_kernels(monkeypatch, cin, ncls, n, hh, ww):
    """Round 5: the fp32 gradient path computes the G tile of separable layers 1 and 2 inside sep_bwd_kernel (UPS template argument) from
    the upper layer's dDW patch -- sep_dx_kernel's arithmetic, tap for tap.  UBD_SEPBWD=split runs the round-4 form (sep_dx_kernel writes
    G, 16-row tiles, dil_wgrad in four waves).  The tiles differ (8 rows vs 16), so weight-gradient sums associate differently: equal to
    rounding, and both inside the autograd tolerance (ragged map sizes included: 72 x 104 and 136 x 200 are no tile multiples)."""
    model, w, x, labels = _setup(cin, ncls, True, n, hh, ww, 77 + cin)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    grads = {}
    for mode in ("fused", "split"):
        if mode == "split":
            monkeypatch.setenv("UBD_SEPBWD", "split")
        m = Model(model.net_config, dtype="float32", seed=0)
        m.set_weights(w)
        tr = Trainer(m, Adam())
        tr.backward_on_device(xt, yt)
        grads[mode] = tr.grads.cpu().numpy().astype(np.float64)
        assert np.isfinite(grads[mode]).all()
    scale = np.abs(grads["split"]).max()
    assert scale > 0
    assert np.abs(grads["fused"] - grads["split"]).max() <= 2e-5 * scale


@pytest.mark.parametrize("cin", [1, 3])
def test_fp32_backward_input_base_not_16_byte_aligned(cin):
    """The 1/3-channel fp32 input patch of the L1 backward kernel is loaded 16 bytes per lane when the base is 16-byte aligned (rows are whole
    chunks: W % 4 == 0); a batch that starts 4 bytes into an allocation takes the element-by-element path.  Same patch, same arithmetic:
    the gradients are bit-identical."""
    model, w, x, labels = _setup(cin, 0, True, 2, 72, 104, 55 + cin)
    tr = Trainer(model, Adam())
    yt = torch.from_numpy(labels).cuda()
    xa = torch.from_numpy(x).cuda()
    tr.backward_on_device(xa, yt)
    g_aligned = tr.grads.clone()
    buf = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    xm = buf[1:1 + x.size].view(x.shape)
    xm.copy_(xa)
    assert xm.data_ptr() % 16 == 4
    tr.backward_on_device(xm, yt)
    assert torch.equal(tr.grads, g_aligned)


def test_adam_step_and_training_reduces_loss():
    model, w, x, labels = _setup(3, 0, True, 4, 64, 64, 21)
    tr = Trainer(model, Adam(lr=1e-3))
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    p0 = model.params.cpu().numpy().astype(np.float64)
    tr.train_step_on_device(xt, yt)
    g = tr.grads.cpu().numpy().astype(np.float64)
    p_ref, _, _ = otorch.adam_step(p0, g, np.zeros_like(g), np.zeros_like(g), 1, lr=1e-3)
    assert np.abs(model.params.cpu().numpy() - p_ref).max() < 1e-6
    first = float(tr.loss[0])
    for _ in range(30):
        tr.train_step_on_device(xt, yt)
    assert float(tr.loss[0]) < first            # the objective goes down on a fixed batch
    assert tr.iterations == 31


def test_train_on_batch_keras_style():
    model, w, x, labels = _setup(1, 2, True, 2, 64, 64, 33)
    tr = Trainer(model)
    loss = tr.train_on_batch(x, labels[..., None])
    ref = otorch.loss_and_grads(x, labels[..., None], w, True)[0]
    assert abs(loss - ref) <= 1e-4 * abs(ref)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("cin,ncls,n,hh,ww", [(3, 0, 3, 72, 104), (1, 3, 2, 64, 96), (3, 2, 8, 128, 128)])
def test_gradients_repeat_bit_for_bit(dtype, cin, ncls, n, hh, ww):
    """Round 4: every block-level sum of the backward pass has a fixed order (wave-sequential LDS adds instead of LDS float atomics in the
    fp32 / fp16 separable backward and in the multi-class head gradient; partial rows totalled in block order): the gradients of
    repeated evaluations are BIT-identical in every activation type, with and without classes.  (The reference makes no such promise --
    TF's reductions are not deterministic; this is what makes fused-vs-split and rank-sum comparisons exact.)"""
    model, w, x, labels = _setup(cin, ncls, True, n, hh, ww, 31 + cin + ncls)
    cfg = model.net_config
    m = Model(cfg, dtype=dtype, seed=0)
    m.set_weights(w)
    tr = Trainer(m, Adam())
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    tr.backward_on_device(xt, yt)
    first = tr.grads.clone()
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    for _ in range(5):
        tr.backward_on_device(xt, yt)
        assert torch.equal(tr.grads, first)
