"""The conditions that make the bit-equality gates of tests/test_gpu_exact16.py and tests/test_gpu_exact_layer32.py fair, checked on the
host with the oracle alone, for every (case, storage type) those files run (tests/exact_cases.py):
  * margin: every stage's sum of |terms| / quantum is below 2^22 -- a condition, two bits under what an fp32 significand holds, so any
    order of summation (and a matrix unit that aligns its addends to the largest one) gives the same bits; fp16 values stay below 2^15
    and at or above 2^-14 (no infinities and no subnormals, whose handling a kernel may legitimately choose);
  * observed: the oracle evaluated in fp32 equals the oracle evaluated in fp64 on the logits and on all nine activations;
  * the outputs are not trivial, every weight is non-zero in some case, every dilated layer has a case whose outputs no storage rounding
    touches, and deliberate faults in the ORACLE (a weight off by one quantum, a halo off by one column, a dropped bias, a truncating
    store, the other padding rule) change the logits -- so equality on these inputs can fail.
Run with -s for the certificate (log2 of the worst ratio) and the positive shares per case and type."""
import numpy as np
import pytest

import exact_cases as ec
from oracle import net_numpy as onet


def test_no_case_was_dropped_and_the_tables_hold_the_required_sizes():
    assert ec.DROPPED == {dt: [] for dt in ec.DTYPES16}
    for size in ((1, 1), (2, 3), (1, 9), (1, 132), (5, 129), (33, 144), (17, 37), (18, 26)):
        assert any((mh, mw) == size for _, mh, mw in ec.CHAIN_MAPS), size
    assert (3, 18, 26) in ec.CHAIN_MAPS and ec.BY_NAME[ec.ONE_CU_CASE].n == 3
    for k in range(6):
        d = ec.DIL[k]
        maps = ec.dense_maps(k)
        assert {(1, 1, 1), (1, 2, 3), (2, 17, 37)} <= set(maps)
        staged = sorted(mw for _, _, mw in maps if -(-mw // d) > 8 and mw != 37)
        assert staged == [8 * d + 1, 8 * d + 2]                        # the two smallest widths with ceil(W4 / d) > 8
    for nm in ec.TRAIN_CASES:
        assert ec.BY_NAME[nm].kind == "chain" and ec.BY_NAME[nm].n_classes == 0
    # the stem runs cover every pair of values of (stem, input form, c_in, padding rule)
    runs = ec.STEM_RUNS
    for a in range(4):
        for b in range(a + 1, 4):
            want = {(u, v) for u in {r[a] for r in runs} for v in {r[b] for r in runs}}
            assert {(r[a], r[b]) for r in runs} == want, (a, b)
    assert {r[0] for r in runs} == {None, "split", "fused12"} and {r[1] for r in runs} == {"u8", "f32", "f32_off4"}
    for _, _, c_in, fml in runs:
        assert len(ec.cases("stem", c_in=c_in, fml=fml)) == len(ec.STEM_MAPS)


@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_exactness_margin_and_observed_exactness(dtype):
    for c in ec.CASES:
        stages = ec.certify(c, dtype)
        lg, acts = ec.reference(c, dtype)
        worst = max(stages, key=lambda s: s.log2_ratio)
        stored = [s for s in stages[:-1]]                               # the head's logits are fp32
        top = max(s.max_stored for s in stored)
        low = min((s.min_stored for s in stored if s.min_stored > 0), default=0.0)
        pos = [float((a > 0).mean()) for a in acts]
        print(f"{c.name:28s} {dtype:8s} worst sum|terms|/quantum 2^{worst.log2_ratio:4.1f} ({worst.name}); stored |a| {low:g}..{top:g}; "
              f"positive {min(pos):.2f}..{max(pos):.2f}; {len(np.unique(lg))} distinct logits of {lg.size}")
        for s in stages:
            assert s.log2_ratio < ec.MARGIN_LOG2, (c.name, s)
        if dtype == "float16":
            assert top < 2.0 ** 15 and (low == 0.0 or low >= 2.0 ** -14), (c.name, low, top)
        lg32, acts32 = ec.reference(c, dtype, "float32")
        assert lg32.dtype == np.float32 and np.array_equal(lg32, lg), c.name
        assert all(np.array_equal(a, b) for a, b in zip(acts32, acts)), c.name
        # not trivial: no dead or saturated layer, no constant map
        assert all(0.2 <= p <= 0.8 for p in pos), (c.name, pos)
        # 16 distinct logits; a map of fewer than 64 logits (1 x 1, 2 x 3, 1 x 9 pixels; half of an identity head's are ReLU zeros) cannot
        # have that many: a quarter of them distinct, and the larger maps of the same family carry the 16
        assert len(np.unique(lg)) >= min(16, max(1, lg.size // 4)), (c.name, len(np.unique(lg)), lg.size)
        if c.name in ec.TRAIN_CASES:
            assert 0.05 <= float((lg[..., 0] > 0).mean()) <= 0.95, c.name   # the train step's counts see both predictions


def test_every_weight_is_non_zero_in_some_case():
    for k in range(6):
        seen = np.zeros((3, 3, ec.C, ec.C), bool)
        for c in ec.cases("dense", layer=k):
            seen |= ec.build(c)[2][9 + 2 * k] != 0
        assert seen.all(), (k, int((~seen).sum()))
    for c_in in (1, 3):
        group = [c for c in ec.CASES if c.c_in == c_in]
        for i in (0, 1, 3, 4, 6, 7):                                   # depthwise and pointwise kernels of L1..L3
            assert np.logical_or.reduce([ec.build(c)[2][i] != 0 for c in group]).all(), (c_in, i)
    heads = [ec.build(c)[2][-2] for c in ec.CASES if c.kind in ("chain", "dense") and c.n_classes == 0]
    assert np.logical_or.reduce([h != 0 for h in heads]).all()


@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_every_dilated_layer_has_a_case_no_storage_rounding_touches(dtype):
    for k in range(6):
        (c,) = ec.cases("small", layer=k)
        s = ec.certify(c, dtype)[6 + k]
        assert s.max_stored > 0 and np.log2(s.max_stored) - s.quantum_log2 < ec.SMALL_LOG2[dtype], (k, s)
        y = ec.reference(c, dtype)[1][3 + k]
        _, xf, w = ec.build(c)
        exact = onet.dilated_conv(ec.reference(c, dtype)[1][2 + k], np.asarray(w[9 + 2 * k], np.float64), np.asarray(w[10 + 2 * k], np.float64), ec.DIL[k])
        assert np.array_equal(y, exact), k                             # the stored output IS the unrounded one


@pytest.mark.parametrize("dtype", ec.DTYPES16)
def test_deliberate_faults_in_the_oracle_change_the_logits(dtype):
    for k in range(6):
        (c,) = ec.cases("dense", layer=k, n_classes=23, mh=17)
        ref = ec.reference(c, dtype)[0]
        for kind in ("weight", "halo", "bias", "truncate"):
            diff = int((ec.mutated_logits(c, dtype, k, kind) != ref).sum())
            print(f"layer {k} {dtype} {kind}: {diff} of {ref.size} logits change")
            assert diff >= 1, (k, kind)
        (c0,) = ec.cases("dense", layer=k, n_classes=0, mh=17)
        assert int((ec.mutated_logits(c0, dtype, k, "weight") != ec.reference(c0, dtype)[0]).sum()) >= 1, k
    (c,) = ec.cases("stem", mh=17, c_in=3, fml=True)
    ref = ec.reference(c, dtype)[0]
    for kind in ("dw", "pw", "padding"):
        diff = int((ec.mutated_stem_logits(c, dtype, kind) != ref).sum())
        print(f"stem {dtype} {kind}: {diff} of {ref.size} logits change")
        assert diff >= 1, kind


def test_the_unmutated_helper_is_the_oracle():
    """mutated_logits re-runs the layers from the stored activations: without a fault it must return the oracle's logits"""
    (c,) = ec.cases("dense", layer=2, n_classes=23, mh=17)
    assert np.array_equal(ec.mutated_logits(c, "bfloat16", 2, None), ec.reference(c, "bfloat16")[0])
    a = np.array([0.0, 1.0, 255.0, 257.0, 1023.5, 3.0 * 2.0 ** -9])
    assert np.array_equal(ec.truncate_to(a, "bfloat16"), [0.0, 1.0, 255.0, 256.0, 1020.0, 3.0 * 2.0 ** -9])


def test_quantum_and_certificate_on_a_hand_made_case():
    assert ec.quantum_log2(np.array([0.0, 6.0, -10.0])) == 1 and ec.quantum_log2(np.array([0.75, 8.0])) == -2
    assert ec.quantum_log2(np.zeros(3)) is None
    w = ec.passthrough(ec.exact_weights(1, 1, 23, 1.0, 0, 1, 0), range(6), True)
    x = np.full((1, 4, 4, 1), 3.0)
    st = ec.certificate(x, w, True, "bfloat16")
    assert st[0].name == "l1.dw" and st[0].quantum_log2 == 0 and st[0].log2_ratio == np.log2(27.0)     # nine taps of |3| * |+-1|
    assert [s.name for s in st] == ["l1.dw", "l1.pw", "l2.dw", "l2.pw", "l3.dw", "l3.pw", "l4", "l5", "l6", "l7", "l8", "l9", "head"]


def test_fp32_layer_cases_are_certified_in_the_winograd_domain():
    w = ec.layer32_weights()
    for shape in ec.LAYER32_SHAPES:
        x = ec.layer32_input(shape)
        assert x.min() < 0 < x.max() or x.size == ec.C
        for k in range(6):
            cert = ec.winograd_certificate(x, w[2 * k], w[2 * k + 1])
            print(f"fp32 layer {k} on {shape}: products 2^{cert.log2_products:.1f}, output transform 2^{cert.log2_output:.1f} quarter quanta; "
                  f"transformed sample {cert.bits_sample} bits, transformed weight {cert.bits_weight} bits")
            assert cert.log2_products < ec.MARGIN_LOG2 and cert.log2_output < ec.MARGIN_LOG2, (shape, k, cert)
            assert cert.bits_sample <= 21 and cert.bits_weight <= 11, (shape, k, cert)
            ref = ec.layer32_reference(shape, k)
            assert np.array_equal(ref, ref.astype(np.float32)) and (shape[1] * shape[2] < 6 or 0.2 <= (ref > 0).mean() <= 0.8), (shape, k)
    assert (w[0] != 0).mean() > 0.7 and all(np.abs(w[2 * k]).max() == 2.0 * 2.0 ** ec.LAYER32_WSCALE[k] for k in range(6))
