"""CPU: the oracle of training through the multi-scale graph (tests/multiscale_train_oracle.py) against itself -- the fuse adjoint is
the adjoint of tests/multiscale_oracle.py's mean, its fp32 restatement agrees with autograd, the composed step at max_scale_power 0 is
oracle.net_torch.loss_and_grads -- and the conditions on the INPUTS that make the gates of tests/test_gpu_multiscale_train.py fair."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import multiscale_oracle as mo  # noqa: E402
import multiscale_train_oracle as mto  # noqa: E402
import train_edge_cases as tc  # noqa: E402
from oracle import net_torch as otorch  # noqa: E402


def _levels(rng, n, mh, mw, k, power, dtype=np.float64):
    return [rng.standard_normal((n, mh >> s, mw >> s, k)).astype(dtype) for s in range(power + 1)]


@pytest.mark.parametrize("power", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 3])
def test_adjoint_identity_fp64(power, k):
    """<fuse(y), g> == <y, fuse_backward(g)> for random y and g"""
    rng = np.random.default_rng(10 * power + k)
    n, mh, mw = 2, 3 << power, 2 << power
    y = _levels(rng, n, mh, mw, k, power)
    g = rng.standard_normal((n, mh, mw, k))
    back = mto.fuse_backward(g, power, dtype=np.float64)
    assert [b.shape for b in back] == [l.shape for l in y]
    lhs = float((mo.fuse_mean_f64(y) * g).sum())
    rhs = float(sum((l * b).sum() for l, b in zip(y, back)))
    scale = float(sum(np.abs(l * b).sum() for l, b in zip(y, back)))
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


@pytest.mark.parametrize("mh,mw,k,power", [(8, 8, 1, 3), (16, 24, 3, 2), (2, 2, 5, 1), (16, 32, 2, 4), (3, 5, 1, 0)])
def test_fp32_adjoint_equals_autograd_of_the_mean(mh, mw, k, power):
    rng = np.random.default_rng(mh + mw + k)
    n = 2
    g = rng.standard_normal((n, mh, mw, k)).astype(np.float32)
    levels = [torch.zeros((n, mh >> s, mw >> s, k), dtype=torch.float64, requires_grad=True) for s in range(power + 1)]
    acc = levels[0]
    for s in range(1, power + 1):                                       # multiscale_oracle.fuse_mean_f64, on torch tensors
        acc = acc + levels[s].repeat_interleave(2 ** s, dim=1).repeat_interleave(2 ** s, dim=2)
    mean = acc / float(power + 1)
    assert np.array_equal(mean.detach().numpy(), mo.fuse_mean_f64([l.detach().numpy() for l in levels]))
    mean.backward(torch.from_numpy(g.astype(np.float64)))
    got = mto.fuse_backward(g, power)
    for s, (a, l) in enumerate(zip(got, levels)):
        want = l.grad.numpy()
        assert a.dtype == np.float32 and a.shape == want.shape
        # a sum of 4^s fp32 terms by a balanced tree of depth 2 s, then one division: (2 s + 1) roundings of at most 2^-24 relative each,
        # taken of the sum of the magnitudes
        mag = mto.fuse_backward(np.abs(g).astype(np.float64), power, dtype=np.float64)[s]
        assert (np.abs(a - want) <= (2 * s + 1) * 2.0 ** -24 * mag * 1.01 + 1e-45).all(), s
    # the levels' values do not enter: the mean is linear
    assert np.array_equal(got[0].view(np.uint32), (g / np.float32(power + 1)).view(np.uint32))


def test_power_zero_oracle_is_the_single_scale_oracle():
    cin, ncls, fml, n, hh, ww, _, seed = mto.STEP_CASES[1]
    w, x, labels = mto.step_inputs(cin, ncls, n, hh, ww, seed)
    loss, logits, dlogits, grads = mto.loss_and_grads(x, labels[..., None], w, True, 0, fml)
    loss_ref, logits_ref, dlogits_ref, grads_ref = otorch.loss_and_grads(x, labels[..., None], w, True, fml)
    assert loss == loss_ref and np.array_equal(logits, logits_ref) and np.array_equal(dlogits, dlogits_ref)
    for a, b in zip(grads, grads_ref):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", mto.STEP_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_fp32_step_cases_mine_clear_of_ties(case):
    """what makes the 1e-3 gate of the GPU test fair: fp32 and fp64 select the same hard negatives"""
    cin, ncls, fml, n, hh, ww, power, seed = case
    w, x, labels = mto.step_inputs(cin, ncls, n, hh, ww, seed)
    with torch.no_grad():
        mean, levels = mto.mean_map(torch.as_tensor(x, dtype=torch.float64), otorch.to_torch_weights(w, torch.float64), power, fml)
    assert tuple(levels[-1].shape[1:3]) == (hh >> (2 + power), ww >> (2 + power))
    k, n_neg, gap = mto.mining_gap(mean.numpy(), labels)
    assert 0 < k < n_neg and gap > mto.MINING_GAP, (k, n_neg, gap)


@pytest.mark.parametrize("dtype", tc.DTYPES16)
def test_16bit_step_case_oracles_agree(dtype):
    """the same-rounding oracle evaluated in fp32 and in fp64: every figure the GPU gates look at, inside a tenth of the tightest gate"""
    case = mto.step16_case()
    loss32, grads32 = mto.step16_reference(dtype, "float32")
    loss64, grads64 = mto.step16_reference(dtype, "float64")
    figures = tc.errors(case, loss32, grads32, loss64, grads64)
    assert max(figures.values()) <= tc.SPREAD_GATE_16BIT, max(figures.items(), key=lambda kv: kv[1])
    w, x, labels = tc.inputs(case, dtype)
    n_pos = int((labels > 0).sum())
    assert 0 < labels.size - n_pos <= n_pos                             # k = n_neg: every negative is taken
