"""GPU: ubd_adam_step (train.hip adam_kernel) against oracle/net_torch.adam_step in float64 on the same fp32 inputs -- all three outputs
(p, m, v), t from 1 to 100 000, grad_scale 1, 1/8 and 1/3, default and non-default hyper-parameters, counts from 1 element to beyond the
1024 x 256 threads of the largest grid (the grid-stride loop), and a chain of 20 steps in which p, m and v feed back.

Bounds, from the kernel's operation count with u = 2^-24 per rounded fp32 operation (division and square root are correctly rounded;
1 - beta is exact for beta >= 1/2; a fused multiply-add only removes roundings).  s = grad_scale, g' = g s (one rounding):
  m = b1 m0 + (1 - b1) g'         product, product of a rounded factor, sum:  |m - m_ref| <= 4u (|b1 m0| + |(1 - b1) g s|) =: 4u M
                                  -- absolute, in the two terms' magnitudes: m cancels, so no bound relative to m itself holds;
  v = b2 v0 + ((1 - b2) g') g'    all terms >= 0, g' enters twice:            |v - v_ref| <= 6u v_ref
  p = p0 - lr_t m / (sqrt(v) + eps)   sqrt of v (3u + u), + eps (u), lr_t m (u), quotient (u), plus m's own 4u M:
                                  |p - p_ref| <= u |p_ref| + 12u lr_t M / (sqrt(v_ref) + eps) + u |update|,
    the last term being the rounding of lr_t itself to fp32 (the library computes it in double).  M stands where the issue's formula has
    |m|: equal where the two terms of m do not cancel, and the only sound reading where they do.
The chain adds the per-step bounds over its steps (m and v errors decay with beta, p's add up); every step is also checked on its own
against one oracle step from the DEVICE's previous state, with the one-step bounds."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import net_torch as otorch
from ubdvss_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEFAULT = (1e-3, 0.9, 0.999, 1e-7)
OTHER = (3e-2, 0.8, 0.99, 1e-5)                                  # lr, beta1, beta2, eps


def _state(rng, count):
    """fp32 p, g, m, v: v >= 0 with exact zeros, some g = 0, and elements with g = m = v = 0"""
    p = rng.normal(0, 0.5, count).astype(np.float32)
    g = (rng.normal(0, 1, count) * 10.0 ** rng.uniform(-4, 1, count)).astype(np.float32)
    m = (rng.normal(0, 1, count) * 10.0 ** rng.uniform(-4, 0, count)).astype(np.float32)
    v = (rng.normal(0, 1, count) ** 2 * 10.0 ** rng.uniform(-8, 1, count)).astype(np.float32)
    v[rng.random(count) < 0.1] = 0.0
    g[rng.random(count) < 0.05] = 0.0
    still = rng.random(count) < 0.05
    still[-1] = count > 1                                       # the last element: the tail of the last block, the end of the stride loop (a single element moves)
    g[still] = 0.0; m[still] = 0.0; v[still] = 0.0
    return p, g, m, v, still


def _step(lib, p, g, m, v, t, hyper, scale):
    lr, b1, b2, eps = hyper
    return lib.ubd_adam_step(p.data_ptr() if p is not None else None, g.data_ptr() if g is not None else None, m.data_ptr() if m is not None else None,
                             v.data_ptr() if v is not None else None, (p if p is not None else g).numel(), t, lr, b1, b2, eps, scale,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _oracle(p, g, m, v, t, hyper, scale):
    """float64 oracle step on the fp32 values the kernel receives (hyper-parameters and grad_scale as the floats the C ABI passes) and the
    one-step bounds"""
    lr, b1, b2, eps = (float(np.float32(h)) for h in hyper)
    s = float(np.float32(scale))
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    p_ref, m_ref, v_ref = otorch.adam_step(p, g * s, m, v, t, lr=lr, beta1=b1, beta2=b2, eps=eps)
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    mag = np.abs(b1 * m) + np.abs((1 - b1) * g * s)
    bound_m = 4 * U * mag
    bound_v = 6 * U * v_ref
    bound_p = U * np.abs(p_ref) + 12 * U * lr_t * mag / (np.sqrt(v_ref) + eps) + U * np.abs(p_ref - p)
    return (p_ref, m_ref, v_ref), (bound_p, bound_m, bound_v)


def _assert_within(got, ref, bounds, tag):
    for name, a, r, b in zip("pmv", got, ref, bounds):
        excess = np.abs(a.astype(np.float64) - r) - b
        i = int(excess.argmax())
        assert excess[i] <= 0, (tag, name, i, float(a[i]), float(r[i]), float(b[i]))


@pytest.mark.parametrize("count", [1, 255, 257, 5209, 300001])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_adam_step_vs_float64(count, t):
    assert 300001 > 1024 * 256 >= 5209                          # the largest count is beyond one pass of the largest grid
    lib = _lib.load()
    rng = np.random.default_rng(1000 * t + count)
    for hyper in (DEFAULT, OTHER):
        for scale in (1.0, 0.125, 1.0 / 3.0):
            p, g, m, v, still = _state(rng, count)
            ref, bounds = _oracle(p, g, m, v, t, hyper, scale)
            dp, dg, dm, dv = (torch.from_numpy(a).cuda() for a in (p, g, m, v))
            assert _step(lib, dp, dg, dm, dv, t, hyper, scale) == 0
            got = [a.cpu().numpy() for a in (dp, dm, dv)]
            assert np.array_equal(dg.cpu().numpy(), g)                               # the gradient is read only
            assert all(np.isfinite(a).all() for a in got)
            _assert_within(got, ref, bounds, (hyper, scale))
            assert np.array_equal(got[0][still].view(np.uint32), p[still].view(np.uint32))   # g = m = v = 0: p keeps its bits
            assert not got[1][still].any() and not got[2][still].any()


def test_adam_chain_of_20_steps():
    lib = _lib.load()
    rng = np.random.default_rng(20)
    count, hyper, scale = 5209, OTHER, 0.125
    p, _, m, v, _ = _state(rng, count)
    m[:] = 0; v[:] = 0                                                # a fresh optimiser
    dp, dm, dv = (torch.from_numpy(a).cuda() for a in (p, m, v))
    rp, rm, rv = (a.astype(np.float64) for a in (p, m, v))           # the pure float64 chain
    sum_bounds = [np.zeros(count), np.zeros(count), np.zeros(count)]
    for t in range(1, 21):
        g = (rng.normal(0, 1, count) * 10.0 ** rng.uniform(-3, 0, count)).astype(np.float32)
        g[rng.random(count) < 0.05] = 0.0
        before = [a.cpu().numpy() for a in (dp, dm, dv)]
        assert _step(lib, dp, torch.from_numpy(g).cuda(), dm, dv, t, hyper, scale) == 0
        got = [a.cpu().numpy() for a in (dp, dm, dv)]
        # this step on its own, from the device's previous state
        ref1, bounds1 = _oracle(before[0], g, before[1], before[2], t, hyper, scale)
        _assert_within(got, ref1, bounds1, ("step", t))
        # the chain
        (rp, rm, rv), bounds = _oracle(rp, g, rm, rv, t, hyper, scale)
        for acc, b in zip(sum_bounds, bounds):
            acc += b
        _assert_within(got, (rp, rm, rv), sum_bounds, ("chain", t))
    assert float(np.abs(got[0] - p).max()) > 0.1                      # twenty steps of lr 3e-2 moved the parameters


def test_adam_rejects_bad_arguments_and_launches_nothing():
    lib = _lib.load()
    rng = np.random.default_rng(3)
    p, g, m, v, _ = _state(rng, 257)
    dev = [torch.from_numpy(a).cuda() for a in (p, g, m, v)]
    assert _step(lib, *dev, 0, DEFAULT, 1.0) != 0                     # t starts at 1
    assert _step(lib, *dev, -3, DEFAULT, 1.0) != 0
    for missing in range(4):
        args = list(dev)
        args[missing] = None
        if missing == 0:                                              # _step takes the count from the first tensor it has
            assert lib.ubd_adam_step(None, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), 257, 1, *DEFAULT, 1.0,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0
        else:
            assert _step(lib, *args, 1, DEFAULT, 1.0) != 0
    torch.cuda.synchronize()
    for a, d in zip((p, g, m, v), dev):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert _step(lib, *dev, 1, DEFAULT, 1.0) == 0                     # and the handle-free call still works afterwards
    assert not np.array_equal(dev[0].cpu().numpy(), p)
