"""The conditions that make the bit-equality gates of tests/test_gpu_exact16.py and tests/test_gpu_exact_layer32.py fair, checked on the
host with the oracle alone, for every (case, storage type) those files run (tests/exact_cases.py):
  * margin: every stage's sum of |terms| / quantum is below 2^22 -- a condition, two bits under what an fp32 significand holds, so any
    order of summation (and a matrix unit that aligns its addends to the largest one) gives the same bits; fp16 values stay below 2^15
    and at or above 2^-14 (no infinities and no subnormals, whose handling a kernel may legitimately choose);
  * observed: the oracle evaluated in fp32 equals the oracle evaluated in fp64 on the logits and on all nine activations;
  * the outputs are not trivial, every weight is non-zero in some case, every dilated layer has a case whose outputs no storage rounding
    touches, and deliberate faults in the ORACLE (a weight off by one quantum, a halo off by one column, a dropped bias, a truncating
    store, the other padding rule) change the logits -- so equality on these inputs can fail.
The fp32 forward cases of tests/test_gpu_exact32.py (exact_cases.CASES32) get the same with no storage rounding, plus the Winograd-domain
condition of every dilated layer on the oracle's own activations and the PIECE LIVENESS of the stem's split products: each of the six kept
(sample piece, weight piece) products of L2's and of L3's pointwise stage is non-zero in some case, the three dropped ones are zero in
every case, and the oracle with one kept product left out returns other logits.
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


# ------------------------------------------------------------------------------------------------ fp32 forward cases (test_gpu_exact32.py)

def test_no_fp32_case_was_dropped_and_the_tables_hold_the_required_sizes():
    assert ec.DROPPED32 == []
    sizes = {(mh, mw) for _, mh, mw in ec.STEM32_MAPS}
    assert {(1, 1), (2, 3), (17, 37), (18, 26)} <= sizes and (2, 17, 37) in ec.STEM32_MAPS and (3, 18, 26) in ec.STEM32_MAPS
    assert {17, 31, 33} <= {mw for _, mw in sizes} and 5 in {mh for mh, _ in sizes}
    assert all(n <= 3 and mh <= 33 and mw <= 144 for c in ec.CASES32 for n, mh, mw in [(c.n, c.mh, c.mw)])
    assert {(c.n, c.mh, c.mw) for c in ec.cases32("chain32")} == set(ec.CHAIN_MAPS) and {c.n_classes for c in ec.cases32("chain32")} == {0, 2}
    assert {c.n_classes for c in ec.cases32("head32")} == {0, 2, 31}
    # the stem runs cover every pair of values of (stem, input form, c_in, padding rule), and every (stem, input form) in full
    runs = ec.STEM32_RUNS
    for a in range(4):
        for b in range(a + 1, 4):
            want = {(u, v) for u in {r[a] for r in runs} for v in {r[b] for r in runs}}
            assert {(r[a], r[b]) for r in runs} == want, (a, b)
    assert {r[0] for r in runs} == {None, "fused123", "cold123", "fused", "unfused"} and {r[1] for r in runs} == {"u8", "f32", "f32_off4"}
    for _, form, c_in, fml in runs:
        group = [c for c in ec.cases32("stem32", c_in=c_in, fml=fml) if form != "u8" or c.setting in ec.U8_SETTINGS]
        assert len(group) == len(ec.STEM32_MAPS) * (len(ec.U8_SETTINGS) if form == "u8" else len(ec.STEM32_SETTINGS))
        assert all((ec.build32(c)[0] is not None) == (c.setting in ec.U8_SETTINGS) for c in group)
    assert set(ec.U8_SETTINGS) >= {"dense", "wide_w2", "wide_w3", "mid2", "mid3"}
    for nm in ec.TRAIN_CASES32 + (ec.ONE_CU_CASE32,):
        assert ec.BY_NAME32[nm].kind == "chain32" and ec.BY_NAME32[nm].n_classes == 0
    assert ec.BY_NAME32[ec.TAIL_CASE32].fml and ec.BY_NAME32[ec.TEETH_PW3_CASE32].fml and ec.BY_NAME32[ec.TEETH_DW2_CASE32].fml
    assert ec.BY_NAME32[ec.TAIL_CASE32].n_classes == 2 and ec.BY_NAME32[ec.TAIL_CASE32].mh == 17


def test_fp32_cases_exactness_margin_observed_exactness_and_winograd_domain():
    """every fp32 (case, form): the forms differ in how the same images reach the device, so one certificate per case covers them"""
    for c in ec.CASES32:
        x8, xf, w = ec.build32(c)
        assert x8 is None or np.array_equal(x8.astype(np.float32), xf)
        stages = ec.certify32(c)
        worst = max(stages, key=lambda s: s.log2_ratio)
        for s in stages:
            assert s.log2_ratio < ec.MARGIN_LOG2, (c.name, s)
        lg, acts = ec.reference32(c)
        lg32, acts32 = ec.reference32(c, "float32")
        assert lg32.dtype == np.float32 and np.array_equal(lg32, lg), c.name
        assert all(np.array_equal(a, b) for a, b in zip(acts32, acts)), c.name
        assert np.array_equal(ec.forward32_mutated(c, None), lg), c.name          # the split-product restatement IS the oracle on these inputs
        wino = [ec.winograd_certificate(acts[2 + k], w[9 + 2 * k], w[10 + 2 * k], per_channel=True) for k in range(6)]
        for k, cert in enumerate(wino):
            assert cert.log2_products < ec.MARGIN_LOG2 and cert.log2_output < ec.MARGIN_LOG2, (c.name, k, cert)
            assert cert.bits_sample <= 22 and cert.bits_weight <= 11, (c.name, k, cert)
        pos = [float((a > 0).mean()) for a in acts[:3 if c.kind != "chain32" else 9]]
        print(f"{c.name:36s} worst sum|terms|/quantum 2^{worst.log2_ratio:4.1f} ({worst.name}); Winograd output 2^{max(x.log2_output for x in wino):4.1f}, "
              f"sample bits {max(x.bits_sample for x in wino)}; positive {min(pos):.2f}..{max(pos):.2f}; {len(np.unique(lg))} distinct logits of {lg.size}")
        # not trivial: no dead or saturated layer (the one-tap, one-term settings leave few positive values on the maps of one to six pixels), no constant map
        assert all(0.05 <= p <= 0.95 for p in pos) or c.mh * c.mw < 6, (c.name, pos)
        assert lg.any() and all(p > 0 for p in pos), (c.name, pos)
        # (a stem of one tap and one term per kernel on 0 / 1 images has one non-zero value per output channel, give or take the bias)
        if c.mh * c.mw >= 6:
            assert len(np.unique(lg)) >= 2, (c.name, len(np.unique(lg)), lg.size)
        if c.name in ec.TRAIN_CASES32:
            assert 0.05 <= float((lg[..., 0] > 0).mean()) <= 0.95, c.name


def test_split3_restatement_on_hand_made_values():
    v = np.array([0.0, 1.0, 255.0, 257.0, 65537.0, 2.0 ** 17 + 3, -(2.0 ** 17 + 3), 2.0 ** 24 - 1, 3.0 * 2.0 ** -9], np.float32)
    p1, p2, p3 = ec.split3(v)
    assert np.array_equal(p1 + p2 + p3, v.astype(np.float64))
    assert np.array_equal(p1, [0, 1, 255, 256, 65536, 2.0 ** 17, -(2.0 ** 17), 2.0 ** 24 - 2.0 ** 16, 3.0 * 2.0 ** -9])
    assert np.array_equal(p2, [0, 0, 0, 1, 1, 3, -3, 2.0 ** 16 - 2.0 ** 8, 0]) and np.array_equal(p3, [0, 0, 0, 0, 0, 0, 0, 255, 0])
    live = ec.split3_certificate(np.array([[257.0, 0.0]]), np.array([[1.0, 0.0], [2.0 ** 23 + 2.0 ** 9 + 1, 0.0]]))
    assert live.tolist() == [[True, False, False], [True, False, False], [False, False, False]]      # channel 1's wide weight meets a zero sample


def test_every_kept_piece_product_is_live_somewhere_and_the_dropped_ones_nowhere():
    seen = [np.zeros((3, 3), bool), np.zeros((3, 3), bool)]
    where = [{}, {}]
    for c in ec.CASES32:
        for layer, live in enumerate(ec.split_liveness32(c)):
            for i, j in ec.DROPPED_PRODUCTS:
                assert not live[i - 1, j - 1], (c.name, f"L{layer + 2}", (i, j))
            seen[layer] |= live
            if c.kind == "stem32":
                for i, j in ec.KEPT:
                    if live[i - 1, j - 1]:
                        where[layer].setdefault((i, j), c.setting)
    for layer in range(2):
        print(f"L{layer + 2}: first setting in which each kept product is live: {where[layer]}")
        for i, j in ec.KEPT:
            assert (i, j) in where[layer], (f"L{layer + 2}", (i, j))
    assert ec.split_liveness32(ec.BY_NAME32[ec.TEETH_PW3_CASE32])[1][0, 2]              # (1, 3) live at L3 in the device-teeth case
    (ci, co), unit = ec.pw3_third_piece_entry(ec.BY_NAME32[ec.TEETH_PW3_CASE32])
    k = ec.build32(ec.BY_NAME32[ec.TEETH_PW3_CASE32])[2][7][0, 0]
    before, after = ec.split3(k[ci, co].reshape(1)), ec.split3(np.float32(k[ci, co] + unit).reshape(1))
    assert before[0] == after[0] and before[1] == after[1] and after[2][0] - before[2][0] == unit == 2.0 ** ec.quantum_log2(k)


def test_every_stem_weight_is_non_zero_in_some_fp32_case():
    for c_in in (1, 3):
        group = ec.cases32("stem32", c_in=c_in)
        for i in (0, 1, 3, 4, 6, 7):
            assert np.logical_or.reduce([ec.build32(c)[2][i] != 0 for c in group]).all(), (c_in, i)
        for i in (2, 5, 8):
            assert np.logical_or.reduce([ec.build32(c)[2][i] != 0 for c in group]).all(), (c_in, i)
    heads = [ec.build32(c)[2][-2] for c in ec.cases32("head32", n_classes=31)]
    assert np.logical_or.reduce([h != 0 for h in heads]).all()


def test_deliberate_faults_in_the_fp32_oracle_change_the_logits():
    """each fault changes the logits of at least one certified case; a piece product that is not live in a case changes nothing there"""
    stem = sorted(ec.cases32("stem32"), key=lambda c: c.n * c.mh * c.mw)
    for layer in (2, 3):
        for ij in ec.KEPT:
            live = [c for c in stem if ec.split_liveness32(c)[layer - 2][ij[0] - 1, ij[1] - 1]]
            hit = next((c.name for c in live if not np.array_equal(ec.forward32_mutated(c, "drop", (layer, ij)), ec.reference32(c)[0])), None)
            print(f"L{layer} without piece product {ij}: live in {len(live)} of {len(stem)} cases, the logits change in {hit}")
            assert hit is not None, (layer, ij)
            dead = next(c for c in stem if c.mh == 17 and c not in live) if ij != (1, 1) else None
            assert dead is None or np.array_equal(ec.forward32_mutated(dead, "drop", (layer, ij)), ec.reference32(dead)[0]), (dead.name, layer, ij)
    stem = ec.cases32("stem32", mh=17)
    for kind in ("dw", "padding", "bias3"):
        diff = [int((ec.forward32_mutated(c, kind) != ec.reference32(c)[0]).sum()) for c in stem]
        print(f"fp32 stem {kind}: logits that change per case {diff}")
        assert max(diff) >= 1, kind
    for c in (ec.BY_NAME32[ec.TEETH_DW2_CASE32],):
        assert int((ec.forward32_mutated(c, "dw") != ec.reference32(c)[0]).sum()) >= 1
    heads = ec.cases32("head32", mh=17) + ec.cases32("chain32", mh=17)
    assert all(int((ec.forward32_mutated(c, "head_bias") != ec.reference32(c)[0]).sum()) >= 1 for c in heads if np.any(ec.build32(c)[2][-1]))
    assert any(np.any(ec.build32(c)[2][-1]) for c in heads)
