"""CPU: the inputs of tests/test_gpu_train_edges.py (tests/train_edge_cases.py) meet the conditions that make the GPU gates fair.  The
conditions are on the INPUTS and are checked with the oracle alone -- nothing here is a measurement of the kernels:
  * the label generator: every class present, a background pixel, n_neg <= n_pos where the case is mined;
  * finite loss, no reference gradient tensor that is exactly zero (none of these cases expects one);
  * cases that are not mined (fp32 only, k < n_neg): the k-th and (k+1)-th largest negative cross-entropies of the fp64 oracle differ by
    more than 1e-3 relative, so kernel and oracle mine the same pixels;
  * every (case, 16-bit type): mined, and the same-rounding oracle evaluated in fp32 and in fp64 agrees on the loss, every gradient
    tensor, every head-kernel column and every head-bias element to one tenth of the gate the GPU test applies; the dropped ones stay
    inside the caps (a fifth of the tiny-map cases per type, no class-count case at 2 x 40 x 36);
  * the class-vote inputs: the two largest mean-softmax votes of every object differ by more than 1e-4 relative (the device sums the votes
    with float atomics in arrival order)."""
import numpy as np
import pytest

import train_edge_cases as tc
from oracle import cv_post as ocv

# reference gradient tensors that are exactly zero, per case: none.  (A class that no pixel carries still has a head gradient: the
# softmax pushes it down.  Whole COLUMNS are zero where there is no positive pixel at all -- errors() compares those exactly.)
EXPECTED_ZERO = {}


def test_case_tables_cover_what_they_claim():
    by_group = lambda g: [c for c in tc.CASES if c.group == g]            # noqa: E731
    cls = by_group("classes")
    for shape in ((2, 40, 36), (1, 64, 96)):
        assert sorted(1 + c.ncls for c in cls if (c.n, c.hh, c.ww) == shape) == [2, 9, 16, 17, 24, 32]
    assert sorted(c.ncls for c in cls if c.one_cu) == [16, 31] and all((c.n, c.hh, c.ww) == (3, 72, 104) for c in cls if c.one_cu)
    assert {c.cin for c in cls} == {1, 3} and {c.fml for c in cls} == {True, False}
    tiny = by_group("tiny")
    assert {(c.hh, c.ww) for c in tiny} == set(tc.TINY_SIDES) | {(4, 4)}
    assert all({c.n for c in tiny if (c.hh, c.ww) == s} == {1, 3} for s in tc.TINY_SIDES)
    assert {c.ncls for c in tiny} == {0, 2, 31} and {c.cin for c in tiny} == {1, 3} and {c.fml for c in tiny} == {True, False}
    assert all(c.n * (c.hh // 4) * (c.ww // 4) > 31 for c in tiny if c.ncls == 31)
    assert {(c.kind, c.ncls) for c in by_group("degenerate")} == {(k, n) for k in ("all_bg", "all_pos", "one_pos") for n in (0, 2)}
    assert all((c.n, c.hh, c.ww) == (2, 8, 12) for c in by_group("degenerate"))
    # 16-bit drops stay inside the caps
    for dt in tc.DTYPES16:
        dropped = tc.DROPPED_16BIT[dt]
        assert not [nm for nm in dropped if nm.endswith("_2x40x36")], dropped
        assert 5 * len([nm for nm in dropped if nm.startswith("tiny_")]) <= len(tiny), dropped
        assert all(tc.BY_NAME[nm].group == "tiny" or tc.BY_NAME[nm].group == "classes" for nm in dropped)
    assert all(c.mined for c, dt in tc.train_runs() if dt != "float32")
    assert all(0 <= c.seeds[dt] <= 31 for c, dt in tc.train_runs() if dt != "float32")


@pytest.mark.parametrize("case,dtype", tc.train_runs(), ids=[f"{c.name}-{dt}" for c, dt in tc.train_runs()])
def test_labels(case, dtype):
    _, x, labels = tc.inputs(case, dtype)
    total = labels.size
    assert labels.shape == (case.n, case.hh // 4, case.ww // 4) and labels.dtype == np.int32
    assert x.dtype == np.float32 and np.abs(x).max() <= 1.0 + 1e-6
    assert labels.min() >= 0 and labels.max() <= max(case.ncls, 1)
    n_pos, n_neg = int((labels > 0).sum()), int((labels == 0).sum())
    if case.kind == "random":
        assert n_neg >= 1 and n_pos >= 1
        if total > case.ncls:
            assert set(np.unique(labels[labels > 0]).tolist()) == set(range(1, max(case.ncls, 1) + 1))
        assert (n_neg <= n_pos) == case.mined
    else:
        assert (n_pos, n_neg) == {"all_bg": (0, total), "all_pos": (total, 0), "one_pos": (1, total - 1)}[case.kind]
    if (case.n, case.hh, case.ww) == (2, 4, 4):
        assert (n_pos, n_neg) == (1, 1)


@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_fp64_reference_is_usable(case):
    loss, _, grads = tc.reference(case)
    assert np.isfinite(loss) and loss > 0
    zero = [nm for nm, g in zip(tc.tensor_names(case), grads) if not np.any(g)]
    assert zero == EXPECTED_ZERO.get(case.name, []), zero
    assert all(np.isfinite(g).all() for g in grads)
    k, n_neg, gap = tc.mining(case)
    if case.mined:
        assert gap is None and k == n_neg                     # every negative is taken
    elif case.kind == "all_pos":
        assert n_neg == 0 and gap is None                     # nothing to mine: the term and its gradient are zero
    else:
        assert k < n_neg and gap > tc.MINING_GAP, (k, n_neg, gap)


_RUNS16 = [(c, dt) for c, dt in tc.train_runs() if dt != "float32"]


@pytest.mark.parametrize("case,dtype", _RUNS16, ids=[f"{c.name}-{dt}" for c, dt in _RUNS16])
def test_same_rounding_oracle_does_not_flip_between_fp32_and_fp64(case, dtype):
    loss, _, grads = tc.reference(case, dtype, "float64")
    assert np.isfinite(loss) and all(np.any(g) for g in grads)
    assert tc.mining(case, dtype)[2] is None
    spread = tc.spread_16bit(case, dtype)
    assert spread <= tc.SPREAD_GATE_16BIT, spread


@pytest.mark.parametrize("n_cls,n,h,w,seed", tc.VOTE_CASES)
def test_class_vote_inputs_have_a_clear_winner(n_cls, n, h, w, seed):
    lg = tc.vote_logits(n_cls, n, h, w, seed)
    margins = tc.vote_margins(lg)
    assert len(margins) >= n and min(m for m, _ in margins) > tc.VOTE_MARGIN, min(m for m, _ in margins)
    # the restatement finds the oracle's objects and winners
    got = []
    for i in range(n):
        got += ocv.postprocess((lg[i, ..., 0] > 0).astype(np.int32), lg[i, ..., 1:], 4, 0)[1].tolist()
    assert sorted(got) == sorted(c for _, c in margins)
    assert len(set(got)) > 2                                    # several different winners, not one class everywhere
    assert max(got) >= 16 or n_cls == 16
