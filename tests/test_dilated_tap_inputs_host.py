"""CPU: the inputs of tests/test_gpu_dilated_taps.py (tests/dilated_tap_cases.py) make its per-tap gates fair, and the per-tap figures
see what the per-tensor ones cannot.  Everything here is the oracle alone -- nothing is a measurement of the kernels:
  * liveness: for every case and type all 54 taps of l4.k .. l9.k and all 27 of l1.dw .. l3.dw are non-zero in the reference gradient;
    at 2 x 64 x 64 exactly 8 of the 9 taps of l8.k are dead (the reason this file exists);
  * the reference's own noise: every figure between the oracle evaluated in fp32 and in fp64, with 1 and with 4 torch threads, stays
    inside a tenth of the gate (1e-4 float32, 2e-3 for the 16-bit types against the same-rounding oracle); the seeds were chosen with
    four renumberings of the hidden channels as further samples (dilated_tap_cases.search_seeds), and the renumbered net is shown to be
    the same function;
  * no (case, type) is dropped; single excluded figures stay inside the caps (named with their spread, at most 2 of the 54 dilated
    taps per (case, type), never a centre tap, never two taps of one layer);
  * mutants of the reference gradient of live17 and ragged33 -- a corner tap of l8.k zeroed, l8.k with ky and kx transposed, a corner
    tap scaled by 1.05, an edge tap of l7.k without the last map row's contributions -- fail the per-tap gate of every type, while the
    scaled corner passes the fp32 per-tensor gate (1e-3) and the zeroed corner the 16-bit per-tensor gates (4e-2 / 3e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dilated_tap_cases as tc
from oracle import net_numpy as onet, net_torch as otorch
from test_gpu_forward16 import TRAIN16_GATE_FP32_SOAK, TRAIN16_GATE_FP64

GATE_GRAD_FP32 = 1e-3                      # tests/test_gpu_train.py
_RUNS = tc.runs()
_IDS = [f"{c.name}-{dt}" for c, dt in _RUNS]


def test_case_table():
    assert [(c.name, c.n, c.hh, c.ww) for c in tc.CASES[:4]] == [("live17", 2, 68, 68), ("ragged33", 1, 132, 80), ("wide260", 1, 68, 1040),
                                                                 ("tall130", 1, 520, 68)]
    assert {c.cin for c in tc.CASES} == {1, 3} and {c.fml for c in tc.CASES} == {True, False}
    assert sorted(c.ncls for c in tc.CASES[:4]) == [0, 0, 0, 2]
    assert set(tc.SEEDS) == {(c.name, dt) for c, dt in _RUNS}           # no (case, type) is dropped
    assert all(0 <= s <= 63 for s in tc.SEEDS.values())
    # the 16 x 16 tiles of dil_wgrad16_kernel / dilconv16s_kernel: sub-grid more than 8 wide and more than 16 high at d = 8 / d = 16
    for name, d in (("block130x65", 8), ("block257x129", 16)):
        c = tc.BY_NAME[name]
        sh, sw = -(-(c.hh // 4) // d), -(-(c.ww // 4) // d)
        assert (sh, sw) == (17, 9)
    assert not any(-(-(c.hh // 4) // d) > 16 and -(-(c.ww // 4) // d) > 8 for c in tc.CASES[:4] for d in (8, 16))


def test_excluded_figures_stay_inside_the_caps():
    for (name, dtype), figs in tc.EXCLUDED.items():
        assert (name, dtype) in tc.SEEDS and tc.search_seeds(tc.BY_NAME[name], dtype, range(64), 1.0) is None
        taps = [nm for nm in figs if nm.startswith(tuple(f"l{li}.k[tap" for li in tc.DIL_LAYERS))]
        assert len(taps) <= 2 and len(taps) == len(figs), figs       # only dilated taps may be left out
        assert not [nm for nm in taps if nm.endswith("[tap 1,1]")], figs
        assert len({nm[:2] for nm in taps}) == len(taps), figs
        assert all(np.isfinite(v) and v > tc.SPREAD_GATE[dtype] for v in figs.values()), figs


@pytest.mark.parametrize("case,dtype", _RUNS, ids=_IDS)
def test_every_tap_is_live(case, dtype):
    loss, logits, grads = tc.reference(case, dtype)
    assert np.isfinite(loss) and loss > 0 and all(np.isfinite(g).all() for g in grads)
    assert tc.dead_taps(case, dtype) == []
    labels = tc.inputs(case, dtype)[2]
    assert (labels == 0).sum() <= (labels > 0).sum()                   # k = n_neg: every negative is mined
    figures = tc.tap_figures(case, loss, grads, loss, grads)
    assert sum(nm.startswith(tuple(f"l{li}.k[tap" for li in tc.DIL_LAYERS)) for nm in figures) == 54
    assert sum(".dw[tap" in nm for nm in figures) == 27
    assert sum(tc.kind_of(nm) == "column" for nm in figures) == 6 * 24
    assert max(figures.values()) == 0.0


@pytest.mark.parametrize("dtype", tc.DTYPES)
def test_favourite_shape_has_eight_dead_taps_in_l8(dtype):
    dead = tc.dead_taps(tc.DEAD_TAPS_CASE, dtype)
    assert sorted(nm for nm in dead if nm.startswith("l8.k")) == sorted(tc.tap_name(8, ky, kx) for ky, kx in tc.TAPS if (ky, kx) != (1, 1))
    # ... and a gradient that is wrong there, or merely non-zero, is an infinite figure, not a small one
    loss, _, grads = tc.reference(tc.DEAD_TAPS_CASE, dtype)
    mutant = [g.copy() for g in grads]
    mutant[tc.tensor_names(tc.DEAD_TAPS_CASE).index("l8.k")][0, 2] = 1e-12
    assert tc.tap_figures(tc.DEAD_TAPS_CASE, loss, mutant, loss, grads)["l8.k[tap 0,2]"] == float("inf")
    assert "l8.k[tap 0,2]" not in tc.tap_figures(tc.DEAD_TAPS_CASE, loss, mutant, loss, grads, live_only=True)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case,dtype", _RUNS, ids=_IDS)
def test_oracle_evaluated_in_fp32_and_fp64_agrees_per_tap(case, dtype, threads):
    figures = tc.gated(case, dtype, tc.spread(case, dtype, threads))
    assert max(figures.values()) <= tc.SPREAD_GATE[dtype], tc.worst(figures, 5)


def test_renumbered_net_is_the_same_function():
    """evaluated in fp64 the renumbered net reproduces the reference: the permutations and their inverse are right"""
    case = tc.BY_NAME["ragged33"]
    assert max(tc.spread_renumbered(case, "float32", 0, evaluated_in="float64").values()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------- mutants
def _l7_tap_without_last_row(case, dtype, ky, kx):
    """(the tap [ky, kx] of l7.k's gradient from the oracle's activations and the gradient at l7's output, the same with the last map
    row of that gradient left out).  The plain fp64 net from layer 7 on is restated in five lines so that z7's gradient can be kept;
    the first value must reproduce the oracle's tap, which checks the restatement."""
    w, x, labels = tc.inputs(case, dtype)
    acts = onet.forward(x.astype(np.float64), w, case.fml, return_all=True)[1]
    tw = otorch.to_torch_weights(w, torch.float64)
    a6 = torch.as_tensor(acts[5]).permute(0, 3, 1, 2)
    t, i, kept = a6, len(tw) - 2 - 2 * 3, None
    for d in otorch.DILATIONS[3:]:
        z = F.conv2d(t, tw[i], tw[i + 1], padding=d, dilation=d)
        if kept is None:
            kept = z.requires_grad_(True)
            z = kept
        t, i = F.relu(z), i + 2
    logits = F.conv2d(t, tw[i], tw[i + 1]).permute(0, 2, 3, 1)
    otorch.total_loss(torch.as_tensor(labels[..., None], dtype=torch.float64), logits, case.ncls > 0).backward()
    gz = kept.grad.permute(0, 2, 3, 1).numpy()                         # (n, mh, mw, co)
    a = acts[5]                                                         # (n, mh, mw, ci)
    d, (n, mh, mw, _) = 8, a.shape
    oy, ox = (ky - 1) * d, (kx - 1) * d

    def tap(rows):
        out = np.zeros((24, 24))
        for y in range(max(0, -oy), min(rows, mh - oy)):
            x0, x1 = max(0, -ox), min(mw, mw - ox)
            out += np.einsum("nxi,nxo->io", a[:, y + oy, x0 + ox:x1 + ox], gz[:, y, x0:x1])
        return out
    return tap(mh), tap(mh - 1)


def _mutants(case, dtype, grads):
    names = tc.tensor_names(case)
    i7, i8 = names.index("l7.k"), names.index("l8.k")

    def with_(i, fn):
        out = list(grads)
        out[i] = grads[i].copy()
        fn(out[i])
        return out

    def zero(g): g[0, 0] = 0
    def scale(g): g[2, 0] *= 1.05
    def transpose(g): g[...] = g.transpose(1, 0, 2, 3).copy()
    out = {"a: corner tap of l8.k zeroed": ("l8.k[tap 0,0]", with_(i8, zero)), "b: l8.k transposed": ("l8.k[tap 0,1]", with_(i8, transpose)),
           "c: corner tap of l8.k x 1.05": ("l8.k[tap 2,0]", with_(i8, scale))}
    # the plain fp64 net on this type's inputs rebuilds the tap; a 16-bit reference loses the same row's (plain) contribution
    full, cut = _l7_tap_without_last_row(case, dtype, 0, 1)
    if dtype == "float32":
        assert np.abs(full - grads[i7][0, 1]).max() <= 1e-9 * np.abs(full).max()
    assert np.any(full != cut)

    def drop(g): g[0, 1] += cut - full
    out["d: edge tap of l7.k without the last map row"] = ("l7.k[tap 0,1]", with_(i7, drop))
    return out


def _failures(case, dtype, loss, grads):
    """what tests/test_gpu_dilated_taps.py gates: {figure: value} above the gate of its type, per-tap and per-column figures only"""
    bad = {}
    for evaluated_in, gate in (("float64", GATE_GRAD_FP32),) if dtype == "float32" else (("float32", TRAIN16_GATE_FP32_SOAK), ("float64", TRAIN16_GATE_FP64[dtype])):
        l_ref, _, g_ref = tc.reference(case, dtype, evaluated_in)
        bad.update({nm: v for nm, v in tc.gated(case, dtype, tc.tap_figures(case, loss, grads, l_ref, g_ref)).items()
                    if tc.kind_of(nm) in ("tap", "column") and not v <= gate})
    return bad


def _tensors_pass(case, dtype, loss, grads, gates):
    """the gates the suite had before: relative L2 per whole tensor"""
    for evaluated_in, gate in gates:
        l_ref, _, g_ref = tc.reference(case, dtype, evaluated_in)
        figures = tc.tap_figures(case, loss, grads, l_ref, g_ref)
        if not all(v <= gate for nm, v in figures.items() if tc.kind_of(nm) == "tensor"):
            return False
    return True


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("name", ["live17", "ragged33"])
def test_mutants_fail_the_per_tap_gates(name, dtype):
    case = tc.BY_NAME[name]
    loss, _, grads = tc.reference(case, dtype)
    assert _failures(case, dtype, loss, grads) == {}                    # the reference itself passes
    mutants = _mutants(case, dtype, grads)
    assert len(mutants) == 4
    for tag, (figure, mutant) in mutants.items():
        bad = _failures(case, dtype, loss, mutant)
        assert figure in bad, (tag, tc.worst(bad, 5))
        assert all(nm.startswith(figure[:4]) for nm in bad), (tag, bad)  # and only figures of the mutated tensor


# where the corner taps of l8.k are a small enough share of the tensor for the per-tensor gates to miss them: on live17 the two left
# corners, [0, 0] and [2, 0], carry 1.0 % of the tensor's norm each in float32 and bfloat16 (the right ones 7 % and 4 %) and 0.3 % with
# float16's seed; on ragged33 every corner carries 5 - 34 %, so the per-tensor gates would notice there
@pytest.mark.parametrize("name", ["live17"])
def test_scaled_corner_tap_passes_the_fp32_per_tensor_gate(name):
    case = tc.BY_NAME[name]
    loss, _, grads = tc.reference(case)
    _, mutant = _mutants(case, "float32", grads)["c: corner tap of l8.k x 1.05"]
    assert _tensors_pass(case, "float32", loss, mutant, [("float64", GATE_GRAD_FP32)])
    assert _failures(case, "float32", loss, mutant)


@pytest.mark.parametrize("dtype", tc.DTYPES16)
@pytest.mark.parametrize("name", ["live17"])
def test_zeroed_corner_tap_passes_the_16bit_per_tensor_gates(name, dtype):
    case = tc.BY_NAME[name]
    loss, _, grads = tc.reference(case, dtype)
    _, mutant = _mutants(case, dtype, grads)["a: corner tap of l8.k zeroed"]
    assert _tensors_pass(case, dtype, loss, mutant, [("float64", TRAIN16_GATE_FP64[dtype]), ("float32", TRAIN16_GATE_FP32_SOAK)])
    assert _failures(case, dtype, loss, mutant)
