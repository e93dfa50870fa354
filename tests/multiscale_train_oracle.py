"""Oracle of training through the multi-scale graph (helper module, not collected).

* ``fuse_backward``: the adjoint of ``multiscale_oracle.fuse_mean_*`` with the arithmetic ``ubd_multiscale_fuse_backward`` fixes
  (include/ubd.h): S_0 = dmean, S_s = (a + b) + (c + d) over the 2 x 2 cells of S_(s-1) -- a, b the upper pair, c, d the lower pair --
  and level s = S_s / (P + 1), every operation rounded to ``dtype`` (numpy fp32: operation for operation what the kernel does).
* ``loss_and_grads``: torch autograd of the whole step, composed from oracle.net_torch alone: ``forward`` on x[:, ::2**s, ::2**s] for
  every level (the pyramid at the sizes the model accepts, tests/test_multiscale_host.py), nearest upsampling with
  ``repeat_interleave``, the per-channel mean, ``total_loss`` on the mean map, ``backward()``.  ``act_dtype`` / ``grad_dtype`` are
  ``net_torch.forward``'s same-rounding options, applied to every level.
* ``mining_gap``: the relative gap between the k-th and the (k+1)-th largest negative cross-entropy of a detection map (None where
  the hard-negative term takes every negative): what decides whether fp32 and fp64 mine the same pixels.
"""
import numpy as np
import torch

from oracle import net_torch as otorch


def fuse_backward(dmean, max_scale_power, dtype=np.float32):
    """dmean: (N, h, w, K), h and w multiples of 2**P -> [level 0, ..., level P], level s (N, h >> s, w >> s, K)"""
    s_prev = np.asarray(dmean, dtype=dtype)
    count = dtype(max_scale_power + 1)
    out = [(s_prev / count).astype(dtype)]
    for _ in range(max_scale_power):
        upper = (s_prev[:, 0::2, 0::2] + s_prev[:, 0::2, 1::2]).astype(dtype)
        lower = (s_prev[:, 1::2, 0::2] + s_prev[:, 1::2, 1::2]).astype(dtype)
        s_prev = (upper + lower).astype(dtype)
        out.append((s_prev / count).astype(dtype))
    return out


def mean_map(x, tw, max_scale_power, fml_compatible=True, act_dtype=None, grad_dtype=None):
    """torch: the multi-scale model's output (N, H/4, W/4, K) and the list of the levels' logits"""
    levels = [otorch.forward(x[:, ::2 ** s, ::2 ** s], tw, fml_compatible, act_dtype, grad_dtype) for s in range(max_scale_power + 1)]
    acc = levels[0]
    for s in range(1, max_scale_power + 1):
        acc = acc + levels[s].repeat_interleave(2 ** s, dim=1).repeat_interleave(2 ** s, dim=2)
    return acc / float(max_scale_power + 1), levels


def loss_and_grads(x, y_true, weights, classification_mode, max_scale_power, fml_compatible=True, dtype=torch.float64, act_dtype=None,
                   grad_dtype=None):
    """As oracle.net_torch.loss_and_grads, for the multi-scale graph: (loss, mean logits, d loss / d mean, [grads in Keras order])."""
    tw = otorch.to_torch_weights(weights, dtype, requires_grad=True)
    xt = torch.as_tensor(np.asarray(x), dtype=dtype)
    yt = torch.as_tensor(np.asarray(y_true), dtype=dtype)
    mean, _ = mean_map(xt, tw, max_scale_power, fml_compatible, act_dtype, grad_dtype)
    mean.retain_grad()
    loss = otorch.total_loss(yt, mean, classification_mode)
    loss.backward()
    return float(loss.detach()), mean.detach().numpy(), mean.grad.numpy().copy(), otorch.from_torch_grads(tw)


def mining_gap(logits, labels):
    """logits: (N, h, w, K) of the oracle; labels (N, h, w).  (k, n_neg, relative gap at rank k or None)"""
    x = np.clip(np.asarray(logits, np.float64)[..., 0], otorch.LOGIT_LO_F32, otorch.LOGIT_HI_F32).reshape(-1)
    z = (np.asarray(labels).reshape(-1) > 0)
    ce = np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))
    neg = np.sort(ce[~z])[::-1]
    k = int(min(max(z.sum(), 1), max((~z).sum(), 1)))
    if k >= neg.size or neg.size == 0:
        return k, int(neg.size), None
    return k, int(neg.size), float((neg[k - 1] - neg[k]) / max(neg[k - 1], 1e-300))


# ---------------------------------------------------------------------------------------------- the step's cases
# fp32 step, (c_in, classes, fml, n, H, W, P, seed): inputs as tests/test_gpu_train.py builds them (weights of `seed` with the head
# kernel x 4, rectangle labels of seed + 1, textured images of seed + 2).  These labels keep k = n_pos < n_neg, so the hard-negative
# term MINES: fp32 (device) and fp64 (oracle) must pick the same k pixels or the gradients differ by a whole pixel's share.  The seed
# of every case is the first from 7 + c_in + classes that mines and whose k-th and (k+1)-th largest negative cross-entropies of the
# fp64 oracle lie more than MINING_GAP apart (fp32 logits agree with fp64 to ~1e-6); tests/test_multiscale_train_host.py holds that on the CPU.
MINING_GAP = 1e-3
STEP_CASES = [(3, 0, True, 2, 64, 64, 3, 11), (1, 3, True, 2, 64, 96, 2, 22), (3, 2, False, 1, 32, 32, 3, 13), (3, 0, True, 1, 64, 128, 4, 26)]


def step_inputs(cin, ncls, n, hh, ww, seed):
    """(weights, fp32 images in [-1, 1], labels (n, hh/4, ww/4))"""
    from oracle import net_numpy as onet
    from ubdvss_amd import synthetic
    w = onet.init_weights(seed, cin, ncls, bias_scale=0.2)
    w[-2] = (w[-2] * 4).astype(np.float32)                    # larger head so that the detection logits are not all tiny
    labels = synthetic.rectangle_maps(seed + 1, n, hh // 4, ww // 4, n_classes=ncls)
    x = synthetic.textured_images(seed + 2, labels, 4, cin).astype(np.float32) / 127.5 - 1.0
    return w, x, labels


# 16-bit step: (3, 2, True, 2, 64, 64, 2) as a tests/train_edge_cases.py case -- scattered labels with n_neg <= n_pos (the hard-negative
# term takes every negative) and, as that module explains for its own table, a seed on which the same-rounding oracle evaluated in
# fp32 and in fp64 agree far inside the gates (storage roundings and ReLUs can flip between two correct evaluations): seed 5 is the
# first of 0..5 where both types agree to better than 1e-5 on every figure (seeds 0, 2, 3 spread up to 2e-2 in one of the types);
# tests/test_multiscale_train_host.py holds SPREAD_GATE_16BIT on the CPU.
STEP16_POWER = 2


def step16_case():
    import train_edge_cases as tc
    return tc.Case("multiscale_2x64x64_p2", "classes", 3, 2, True, 2, 64, 64, True, "random", False, {"bfloat16": 5, "float16": 5, "float32": 5})


_REFERENCE16 = {}


def step16_reference(dtype, evaluated_in):
    """(loss, [gradients]) of the same-rounding multi-scale oracle; computed once per process, callers do not write into it.  One
    torch thread, as tests/train_edge_cases.reference."""
    import train_edge_cases as tc
    key = (dtype, evaluated_in)
    if key not in _REFERENCE16:
        case = step16_case()
        w, x, labels = tc.inputs(case, dtype)
        before = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            loss, _, _, grads = loss_and_grads(x, labels[..., None], w, True, STEP16_POWER, case.fml, getattr(torch, evaluated_in), dtype,
                                               "bfloat16" if dtype == "bfloat16" else None)
        finally:
            torch.set_num_threads(before)
        _REFERENCE16[key] = (loss, grads)
    return _REFERENCE16[key]
