"""Case table, inputs, references and figures of the per-tap checks of the dilated layers' weight gradients (helper module, not
collected).  Shared by tests/test_dilated_tap_inputs_host.py (CPU: the conditions on the INPUTS that make the GPU gates fair, and the
proof that the per-tap figures see what the per-tensor ones cannot, with the oracle alone) and tests/test_gpu_dilated_taps.py (the
kernels against the oracle on those inputs).

Why per tap: a tap at offset +-d of a layer with dilation d contributes only where the map is larger than d.  On a 16 x 16 map eight of
the nine taps of l8.k (d = 16) are exactly zero in the reference gradient, and where they are live a tap fed by one map row or column
carries about a hundredth of the tensor's norm: a per-tensor relative L2 lets a wrong off-centre tap through.

Cases (n x H x W -> quarter-resolution map), the smallest shapes that reach the code in question:

  live17        2 x   68 x   68   17 x  17  every tap of every dilation is live; the d = 16 sub-grids are 2 x 2 and 1 x 1 pixels: off-centre
                                            taps of l8 see one row or column, corner taps one pixel per image
  ragged33      1 x  132 x   80   33 x  20  ragged at every resolution; d = 16 sub-grids 3 x 2, d = 8 sub-grids 5 x 3; five tile rows at d = 1
  wide260       1 x   68 x 1040   17 x 260  d = 16 sub-grid 2 x 17: two 16-wide tile columns, the second one pixel wide; d = 8: 3 x 33 (three
                                            columns); d = 4: 5 x 65 (five)
  tall130       1 x  520 x   68  130 x  17  d = 16 sub-grid 9 x 2: two 8-row tile rows, the second one row high; d = 8: 17 x 3 (three rows)
  block130x65   1 x  520 x  260  130 x  65  see below: d = 8 sub-grid 17 x 9, the second tile ROW of the 16 x 16 tiles
  block257x129  1 x 1028 x  516  257 x 129  see below: d = 16 sub-grid 17 x 9, the same at the largest dilation

Tile constants of the other kernels on this path, read before the table was fixed:
  * dil_wgrad_kernel (bwd32.hip; fp32 and fp16): 8 x 16 tiles of a phase sub-grid -- the first four cases cross both boundaries at
    d = 8 and d = 16.
  * Winograd data gradient (wino.hip): a wave's group is 16 tiles = 16 "left-half" columns x one row, columns x / x + d and rows
    y / y + d forming a tile, so the groups repeat every 2 d = 32 columns and rows at d = 16: wide260 has nine column blocks, tall130 five
    row blocks; ragged33 ends inside a block in both directions.
  * dil_wgrad16_kernel (bwd16.h; bf16): TW = 8 (8 x 8 tiles) where the sub-grid is at most 8 columns wide, otherwise TW = 16 with
    W16_TH = 16 ROWS.  tall130 (17 columns: sub-grids 2 and 3 wide) only ever meets the 8-row form; the 16 x 16 form gets a second
    tile row only where the sub-grid is more than 8 wide AND more than 16 high: d = 8 needs a map above 128 x 64, d = 16 above 256 x 128.
  * dilconv16s_kernel (fwd16.hip; the staged 16-bit forward kernel): 16 x 16 tiles, taken where the sub-grid is more than 8 wide --
    the same two boundaries.
  None of the first four shapes crosses them, so block130x65 and block257x129 are the smallest maps that do (129 / 257 rows would do;
  130 keeps tall130's height).  They also give dil_wgrad_kernel two tile columns AND rows in one launch.
  * PAIR items of dil_wgrad16_kernel (two sub-grids exactly 8 wide side by side, d = 16 on 128-wide maps) are an item form, not a tile
    boundary; tests/test_gpu_forward16.py compares them with the 8-wide form.

Grey / RGB and the two padding rules alternate; the class count is 0 except for ragged33 (2 classes).

Inputs per (case, type), from ONE seed: weights onet.init_weights(seed, cin, ncls, bias_scale=0.2) with the head kernel x 4 (as
tests/test_gpu_train.py builds them), labels soak_labels.mostly_positive_maps (seed + 1) for every type -- k = n_neg, the mined term
takes every negative and the comparison is continuous; with sparse rectangles a near-tie at the k-th negative moved one tensor by 1.9e-3
between two evaluations of the ORACLE -- and images synthetic.textured_images (seed + 2) over those labels.

Seeds: a 16-bit storage rounding or a ReLU can flip between two correct evaluations that accumulate differently, and a tap fed by a few
pixels -- or the column of a channel that is alive on a few dozen pixels -- moves by percents with one flip.  A seed qualifies for a type
when every figure of tap_figures() between the oracle evaluated in fp32 and in fp64 stays inside a tenth of the tightest gate the GPU
test applies (1e-4 for float32 against the plain net, 2e-3 for the 16-bit types against the same-rounding net)
  * under 1 and under 4 torch threads (spread()), and
  * with the hidden channels of the net renumbered, RENUMBERINGS = 4 fixed sets of permutations (spread_renumbered()): the same function,
    every sum over channels in another order.  One fp32-against-fp64 pair is ONE sample of where the flips fall and misses most of them:
    block130x65 / float16 / seed 1 passed it at 5e-4, while l4.k[:, :, :, 20] -- a channel alive on 41 of 8450 pixels -- moves by 4e-2 and
    8e-2 in two of six renumbered evaluations of the oracle; the kernels, a further sample, were 2.4e-2 (one pixel of 41) off there and
    inside 5e-4 on the other 248 figures.  (Perturbing the IMAGES instead is not a fair sample: their saturated stripes make many
    depthwise sums exact rounding ties, which oracle and kernels round alike and a perturbation breaks.)
SEEDS stores the first seed of 0..63 that qualifies with half that margin (0..31 sufficed for all but tall130 and block257x129 in
bfloat16: seeds 34 and 46); search_seeds() re-derives an entry on the machine the table was made on -- an fp32 evaluation of the oracle
depends on the machine's convolution code, so elsewhere the renumbered samples fall differently (ragged33 / bfloat16 showed 1.2e-2 on
the nine values of a grey l1.dw in one of them on another CPU); the tests therefore assert the two-thread condition, which held on
both, and that the renumbered net is the same function.  No (case, type) is dropped and EXCLUDED (single figures left out, with
their spread) is empty: every entry qualified whole.
"""
import collections
import functools

import numpy as np

import soak_labels
from oracle import net_numpy as onet, net_torch as otorch
from ubdvss_amd import synthetic

DTYPES = ("float32", "bfloat16", "float16")
DTYPES16 = DTYPES[1:]
SPREAD_GATE_FP32 = 1e-4             # one tenth of the 1e-3 gate against fp64 autograd
SPREAD_GATE_16BIT = 2e-3            # one tenth of the 2e-2 gate against the fp32-evaluated same-rounding oracle
SPREAD_GATE = {"float32": SPREAD_GATE_FP32, "bfloat16": SPREAD_GATE_16BIT, "float16": SPREAD_GATE_16BIT}
DIL_LAYERS = tuple(range(4, 10))
SEP_LAYERS = (1, 2, 3)
TAPS = tuple((ky, kx) for ky in range(3) for kx in range(3))

Case = collections.namedtuple("Case", "name cin ncls fml n hh ww")

CASES = (
    Case("live17", 3, 0, True, 2, 68, 68),
    Case("ragged33", 1, 2, False, 1, 132, 80),
    Case("wide260", 3, 0, False, 1, 68, 1040),
    Case("tall130", 1, 0, True, 1, 520, 68),
    Case("block130x65", 3, 0, True, 1, 520, 260),
    Case("block257x129", 1, 0, False, 1, 1028, 516),
)
BY_NAME = {c.name: c for c in CASES}
DEAD_TAPS_CASE = Case("dead64", 3, 0, True, 2, 64, 64)          # the suite's favourite shape: 8 of the 9 taps of l8.k do not exist

# first seed of 0..63 that qualifies with half the margin, per (case, type): search_seeds(case, dtype)
SEEDS = {
    ("live17", "float32"): 0, ("live17", "bfloat16"): 0, ("live17", "float16"): 4,
    ("ragged33", "float32"): 0, ("ragged33", "bfloat16"): 3, ("ragged33", "float16"): 1,
    ("wide260", "float32"): 0, ("wide260", "bfloat16"): 10, ("wide260", "float16"): 0,
    ("tall130", "float32"): 0, ("tall130", "bfloat16"): 34, ("tall130", "float16"): 0,
    ("block130x65", "float32"): 1, ("block130x65", "bfloat16"): 9, ("block130x65", "float16"): 20,
    ("block257x129", "float32"): 1, ("block257x129", "bfloat16"): 46, ("block257x129", "float16"): 20,
}
# (case, type) -> {figure name: measured spread}: figures left out because no seed of 0..63 qualified the (case, type) whole
EXCLUDED = {}


def seed_of(case, dtype):
    return SEEDS.get((case.name, dtype), 7)


def weights_of(case, seed):
    w = onet.init_weights(seed, case.cin, case.ncls, bias_scale=0.2)
    w[-2] = (w[-2] * 4).astype(np.float32)                    # larger head so that the logits are not all tiny
    return w


def labels_of(case, seed):
    return soak_labels.mostly_positive_maps(np.random.default_rng(seed + 1), case.n, case.hh // 4, case.ww // 4, case.ncls)


def inputs(case, dtype="float32", seed=None):
    """(weights, fp32 images in about [-1, 1], labels) of the case for one activation type"""
    seed = seed_of(case, dtype) if seed is None else seed
    labels = labels_of(case, seed)
    x = synthetic.textured_images(seed + 2, labels, 4, case.cin).astype(np.float32) / 127.5 - 1.0
    return weights_of(case, seed), x, labels


def reference(case, dtype="float32", evaluated_in="float64", threads=1, seed=None):
    """(loss, logits, [gradients in Keras order]) of the oracle on inputs(case, dtype): the plain net for float32, the same-rounding net
    (activations, kernels and -- bf16 -- gradient tensors rounded as the kernels store them) for a 16-bit type.  Computed once per
    process and shared; callers do not write into it."""
    return _reference(case, dtype, evaluated_in, threads, seed_of(case, dtype) if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _reference(case, dtype, evaluated_in, threads, seed):
    import torch
    w, x, labels = inputs(case, dtype, seed)
    act = None if dtype == "float32" else dtype
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        loss, logits, _, grads = otorch.loss_and_grads(x, labels[..., None], w, case.ncls > 0, case.fml, dtype=getattr(torch, evaluated_in),
                                                       act_dtype=act, grad_dtype="bfloat16" if dtype == "bfloat16" else None)
    finally:
        torch.set_num_threads(before)
    return loss, logits, grads


def tensor_names(case):
    return [nm for nm, _ in onet.weight_shapes(case.cin, case.ncls)]


def split_flat(flat, grads_ref):
    """the flat gradient vector of the device as a list of tensors shaped like the reference's"""
    out, off = [], 0
    for gr in grads_ref:
        out.append(np.asarray(flat[off:off + gr.size]).reshape(gr.shape))
        off += gr.size
    assert off == flat.size
    return out


def _fig(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.linalg.norm(b)
    if s == 0:
        return 0.0 if not np.any(a) else float("inf")
    return float(np.linalg.norm(a - b) / s)


def tap_name(layer, ky, kx):
    return f"l{layer}.{'k' if layer >= 4 else 'dw'}[tap {ky},{kx}]"


def column_name(layer, co):
    return f"l{layer}.k[:, :, :, {co}]"


def tap_figures(case, loss, grads, loss_ref, grads_ref, live_only=False):
    """Every figure the gates look at, of a flat gradient vector or a list of tensors against a reference list:
      'loss'                  relative error of the loss
      tensor name             relative L2 of the whole tensor
      'l8.k[tap ky,kx]'       relative L2 of one tap of a 3 x 3 kernel: a 24 x 24 slice of l4.k .. l9.k, a cin vector of l1.dw .. l3.dw
      'l8.k[:, :, :, co]'     relative L2 of one output-channel column of l4.k .. l9.k (216 values)
    A figure whose reference is exactly zero is 0.0 if the other side is exactly zero too and inf otherwise (live_only leaves those
    figures out instead: for shapes on which some taps do not exist)."""
    if isinstance(grads, np.ndarray):
        grads = split_flat(grads, grads_ref)
    out = {"loss": abs(loss - loss_ref) / abs(loss_ref)}

    def put(name, a, b):
        if not (live_only and not np.any(b)):
            out[name] = _fig(a, b)
    by_name = {}
    for nm, g, gr in zip(tensor_names(case), grads, grads_ref):
        assert g.shape == gr.shape, (nm, g.shape, gr.shape)
        put(nm, g, gr)
        by_name[nm] = (g, gr)
    for layer in SEP_LAYERS + DIL_LAYERS:
        g, gr = by_name[f"l{layer}.{'k' if layer >= 4 else 'dw'}"]
        for ky, kx in TAPS:
            put(tap_name(layer, ky, kx), g[ky, kx], gr[ky, kx])
        if layer >= 4:
            for co in range(gr.shape[3]):
                put(column_name(layer, co), g[..., co], gr[..., co])
    return out


def kind_of(name):
    return "loss" if name == "loss" else "tap" if "[tap" in name else "column" if "[:" in name else "tensor"


def gated(case, dtype, figures):
    """the figures without the ones EXCLUDED for this (case, type)"""
    skip = EXCLUDED.get((case.name, dtype), {})
    return {nm: v for nm, v in figures.items() if nm not in skip}


def worst(figures, count=10):
    """the `count` largest figures with their names, largest first"""
    return sorted(figures.items(), key=lambda kv: -kv[1] if kv[1] == kv[1] else -np.inf)[:count]


def dead_taps(case, dtype="float32", seed=None):
    """names of the 3 x 3 taps whose reference gradient is exactly zero"""
    _, _, grads = reference(case, dtype, "float64", 1, seed)
    by_name = dict(zip(tensor_names(case), grads))
    return [tap_name(layer, ky, kx) for layer in SEP_LAYERS + DIL_LAYERS for ky, kx in TAPS
            if not np.any(by_name[f"l{layer}.{'k' if layer >= 4 else 'dw'}"][ky, kx])]


def spread(case, dtype, threads=1, seed=None):
    """tap_figures() between the oracle of this type evaluated in fp32 (with `threads` torch threads) and in fp64"""
    l32, _, g32 = reference(case, dtype, "float32", threads, seed)
    l64, _, g64 = reference(case, dtype, "float64", 1, seed)
    return tap_figures(case, l32, g32, l64, g64)


RENUMBERINGS = 4


def renumbered(tensors, perms, inverse=False):
    """Weights of the SAME net with the 24 channels of hidden layer i renumbered by perms[i] (nine permutations); inverse: gradients of
    the renumbered net back in the original numbering.  The function the net computes does not change, the order of every sum over
    channels does."""
    take = [np.argsort(p) if inverse else np.asarray(p) for p in perms]
    out, i = [], 0
    for li in range(9):
        if li < 3:
            dw, pw, b = tensors[i:i + 3]
            if li:
                dw, pw = dw[:, :, take[li - 1], :], pw[:, :, take[li - 1], :]
            out += [dw, pw[..., take[li]], b[take[li]]]
            i += 3
        else:
            k, b = tensors[i:i + 2]
            out += [k[:, :, take[li - 1], :][..., take[li]], b[take[li]]]
            i += 2
    out += [tensors[i][:, :, take[8], :], tensors[i + 1]]
    return [np.ascontiguousarray(t) for t in out]


def spread_renumbered(case, dtype, which, seed=None, evaluated_in="float32"):
    """tap_figures() between the oracle with its hidden channels renumbered (permutation set `which` of RENUMBERINGS), evaluated in
    fp32, and reference(): one more sample of what the summation order alone does to the figures (see the module docstring).  Evaluated
    in fp64 the renumbered net reproduces reference() to 1e-14.  Like every fp32 evaluation of the oracle, the sample depends on the
    machine's convolution code: it serves search_seeds(), the tests do not assert it."""
    import torch
    seed = seed_of(case, dtype) if seed is None else seed
    w, x, labels = inputs(case, dtype, seed)
    rng = np.random.default_rng(1000 + which)
    perms = [rng.permutation(onet.N_FILTERS) for _ in range(9)]
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        loss, _, _, grads = otorch.loss_and_grads(x, labels[..., None], renumbered(w, perms), case.ncls > 0, case.fml, dtype=getattr(torch, evaluated_in),
                                                  act_dtype=None if dtype == "float32" else dtype, grad_dtype="bfloat16" if dtype == "bfloat16" else None)
    finally:
        torch.set_num_threads(before)
    l64, _, g64 = reference(case, dtype, "float64", 1, seed)
    return tap_figures(case, loss, renumbered(grads, perms, inverse=True), l64, g64)


def search_seeds(case, dtype, candidates=range(64), margin=0.5):
    """Re-derives a table entry: the first seed whose reference has every tap live and whose spread() under 1 and 4 threads and
    spread_renumbered() under every permutation set stay inside `margin` of the type's spread gate (None: no candidate qualifies)."""
    for s in candidates:
        ok = (not dead_taps(case, dtype, s) and all(max(spread(case, dtype, t, s).values()) <= margin * SPREAD_GATE[dtype] for t in (1, 4))
              and all(max(spread_renumbered(case, dtype, k, s).values()) <= margin * SPREAD_GATE[dtype] for k in range(RENUMBERINGS)))
        _reference.cache_clear()
        if ok:
            return s
    return None


def runs():
    return [(c, dt) for c in CASES for dt in DTYPES]
