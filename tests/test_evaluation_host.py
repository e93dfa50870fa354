"""CPU: the exact oracle of the evaluation tests against closed forms and a hand-worked matching, FtMetrics against
hand-computed sums, the scalar_logs key set, the host-side ValueErrors, and no CPU path for the device entry points."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import eval_cases as ec  # noqa: E402
import eval_oracle as eo  # noqa: E402
from ubdvss_amd import NetConfig, ObjectMarkup  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402


def R(x0, y0, x1, y1):
    return eo.poly([x0, y0, x1, y0, x1, y1, x0, y1])


def test_oracle_areas_against_closed_forms():
    a = R(0, 0, 10, 6)
    assert eo.area(a) == 60 and eo.area(eo.poly([0, 0, 0, 6, 10, 6, 10, 0])) == 60          # either winding
    assert eo.area(eo.poly([0, 0, 4, 0, 0, 3])) == 6
    assert eo.intersection(a, R(20, 0, 30, 6)) == 0                                          # disjoint
    assert eo.intersection(a, R(2, 1, 5, 4)) == 9                                            # nested
    assert eo.intersection(a, a) == 60 and eo.iou_of(60, 60, eo.intersection(a, a)) == 1     # identical
    assert eo.intersection(a, R(10, 0, 20, 6)) == 0                                          # sharing an edge
    assert eo.intersection(a, R(10, 6, 12, 8)) == 0                                          # touching in a corner
    assert eo.intersection(a, R(4, -2, 14, 3)) == 18
    # a square of side 2 against its 45-degree turn (half diagonal sqrt 2 is irrational: take the turn of the square of
    # half diagonal 2, i.e. |x| + |y| <= 2, against |x|, |y| <= 3/2): the octagon 9 - 4 * (1/2) = 7
    sq, diamond = R(Fr(-3, 2), Fr(-3, 2), Fr(3, 2), Fr(3, 2)), eo.poly([2, 0, 0, 2, -2, 0, 0, -2])
    assert eo.intersection(sq, diamond) == 7
    assert eo.area_sets([sq, diamond]) == 9 + 8 - 7
    # quarter-pixel coordinates stay exact
    assert eo.intersection(R(0, 0, 2.25, 1.5), R(1.75, 0.25, 5, 5)) == Fr(1, 2) * Fr(5, 4)


def test_oracle_unions_with_coincident_edges():
    a, b, c = R(0, 0, 10, 10), R(10, 0, 20, 10), R(5, 0, 15, 10)
    assert eo.area_sets([a, b]) == 200                                   # a shared edge, opposite directions
    assert eo.area_sets([a, c]) == 150                                   # collinear edges of the same direction
    assert eo.area_sets([a, a, a]) == 100                                # identical polygons
    assert eo.area_sets([a, b, c]) == 200
    assert eo.area_sets([a, R(10, 10, 12, 12)]) == 104                   # a shared vertex
    assert eo.area_sets([a, eo.poly([0, 0, 5, 0, 10, 0, 5, 0])]) == 100   # a zero-area sliver covers nothing
    assert eo.area_sets([a, b], [c]) == 100                              # a union against a box
    assert eo.area_sets([a], [b, c]) == 50
    assert eo.area_sets([], [a]) == 0 and eo.area_sets([]) == 0


def _counts(T, thr):
    o = T.analyze(thr)
    return (o["tp"], o["fp"], o["fn"], o["one_to_one"], o["one_to_many"], o["many_to_one"], o["matched_boxes_count"], o["detection_rate"])


def test_oracle_one_to_many_worked_by_hand():
    """A 100 x 10 ground truth, found as 60 x 10 and 30 x 10 pieces: pair IoUs 0.6 and 0.3 (> 0.05: adjacent), group union 900,
    group IoU 900 / 1000 = 0.9; a far false positive.  By area: intersection 900, found 900 + 100, ground truth 1000: IoU 9/11."""
    T = eo.Tables([R(0, 0, 100, 10)], [R(0, 0, 60, 10), R(70, 0, 100, 10), R(500, 500, 510, 510)])
    assert T.iou[0] == [Fr(3, 5), Fr(3, 10), 0]
    assert [m[2] for m in T.one_to_manys] == [Fr(9, 10)] and not T.one_to_ones and not T.many_to_ones
    assert T.iou_by_area == Fr(900, 1100) and T.precision_by_area == Fr(9, 10) and T.recall_by_area == Fr(9, 10)
    for thr in ev.DatasetMetricCalculator.IOU_THRESHOLDS:
        accepted = Fr(9, 10) >= Fr(float(thr))
        rate = 1 if Fr(9, 11) > Fr(float(thr)) else 0
        assert _counts(T, thr) == ((1, 1, 0, 0, 1, 0, 1, rate) if accepted else (0, 3, 1, 0, 0, 0, 0, rate)), float(thr)
    assert Fr(9, 10) < Fr(0.9) and _counts(T, 0.9) == (0, 3, 1, 0, 0, 0, 0, 0)       # the double 0.9 is 2.2e-17 above 9/10: rejected
    assert _counts(T, 0.85) == (1, 1, 0, 0, 1, 0, 1, 0)
    o = T.analyze(0.5, [1], [0, 2, 1], 3)                                # weights inter / sum(inter) = 600/900, 300/900
    assert o["confusion"][1] == [Fr(2, 3), 0, Fr(1, 3)] and o["iou_sum"] == Fr(9, 10)


def test_oracle_many_to_one_and_the_asymmetries_worked_by_hand():
    """Two 40 x 10 ground truths side by side (a gap of 10), one 90 x 10 found quad over both: pair IoU 400 / 900 each; group
    union 800 inside the quad: IoU 800 / 900 = 8/9."""
    T = eo.Tables([R(0, 0, 40, 10), R(50, 0, 90, 10)], [R(0, 0, 90, 10)])
    assert [m[2] for m in T.many_to_ones] == [Fr(8, 9)] and not T.one_to_ones and not T.one_to_manys
    for thr in ev.DatasetMetricCalculator.IOU_THRESHOLDS:
        rate = 1 if Fr(8, 9) > Fr(float(thr)) else 0
        assert _counts(T, thr) == ((2, 0, 0, 0, 0, 2, 1, rate) if Fr(8, 9) >= Fr(float(thr)) else (0, 1, 2, 0, 0, 0, 0, rate))
    assert T.analyze(0.5, [0, 2], [1], 3)["confusion"] == [[0, 1, 0], [0, 0, 0], [0, 1, 0]]
    # a third ground truth also touched by a second found quad that touches the first ground truth too: the first ground truth
    # has two found quads, one of which has two ground truths -> no 1-many; the quads have ground truths with two quads -> no many-1
    T = eo.Tables([R(0, 0, 100, 10), R(110, 0, 200, 10)], [R(0, 0, 60, 10), R(60, 0, 190, 10)])
    assert T.broken_one_to_many == 1 and not T.one_to_manys and not T.many_to_ones and not T.one_to_ones
    assert _counts(T, 0.4)[:3] == (0, 2, 2)
    # 1-1 below the threshold: a miss and a false positive; IoU exactly 1/2 is accepted at 0.5 and is no detection there
    g, f = ec.tie_image()
    T = eo.Tables([eo.poly(p) for p in g], [eo.poly(p) for p in f])
    assert T.iou == [[Fr(1, 2)]] and _counts(T, 0.5) == (1, 0, 0, 1, 0, 0, 1, 0) and _counts(T, 0.55) == (0, 1, 1, 0, 0, 0, 0, 0)
    # no found objects
    assert _counts(eo.Tables([R(0, 0, 5, 5)], []), 0.4) == (0, 0, 1, 0, 0, 0, 0, 0)


def test_listed_images_are_valid_input():
    for i, (g, f) in enumerate(ec.listed_images()):
        for o, p in enumerate(g):
            ev.check_ground_truth_polygon(p, i, o)
            assert eo.is_convex(eo.poly(p))
        assert all(len(q) == 8 and all(isinstance(v, int) for v in q) for q in f)
    for seed, quant in ((ec.SEED_INT, 1), (ec.SEED_QUARTER, 0.25)):
        for g, f in ec.batch(seed, quant, with_listed=False):
            assert all(abs(v) < 2 ** 14 and v * 4 == int(v * 4) for p in g + f for v in p)


def _metrics(tp, fp, fn, o2o, o2m, m2o, avg_iou, boxes, p, r, i, rate, images=1):
    m = ev.FtMetrics()
    m.tp, m.fp, m.fn, m.one_to_one, m.one_to_many, m.many_to_one = tp, fp, fn, o2o, o2m, m2o
    m.average_iou, m.matched_boxes_count = avg_iou, boxes
    m.average_precision_by_area, m.average_recall_by_area, m.average_iou_by_area, m.detection_rate = p, r, i, rate
    m.matched_images_count = images
    return m


def test_ftmetrics_append_and_reports_against_hand_sums():
    total = ev.FtMetrics()
    assert total.get_metrics() == (0, 0, 0)
    total.append(_metrics(3, 1, 0, 2, 1, 0, 0.8, 3, 0.9, 0.7, 0.6, 1))
    total.append(_metrics(1, 0, 3, 1, 0, 0, 0.6, 1, 0.5, 0.3, 0.2, 0))
    total.append(_metrics(0, 2, 1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0))
    assert (total.tp, total.fp, total.fn, total.one_to_one, total.one_to_many, total.many_to_one) == (4, 3, 4, 3, 1, 0)
    assert total.matched_boxes_count == 4 and total.matched_images_count == 3
    assert total.average_iou == pytest.approx((0.8 * 3 + 0.6) / 4, abs=1e-15)
    assert total.average_precision_by_area == pytest.approx(1.4 / 3, abs=1e-15)
    assert total.average_recall_by_area == pytest.approx(1.0 / 3, abs=1e-15)
    assert total.average_iou_by_area == pytest.approx(0.8 / 3, abs=1e-15)
    assert total.detection_rate == pytest.approx(1 / 3, abs=1e-15)
    p, r, f1 = total.get_metrics()
    assert (p, r) == (4 / 7, 4 / 8) and f1 == pytest.approx(2 * (4 / 7) * 0.5 / (4 / 7 + 0.5), abs=1e-15)
    assert total.get_report() == ('pr = 0.5714, r = 0.5000, f1 = 0.5333 [tp = 4 = 3 (1-1) + 1 (1-m) + 0 (m-1); fp = 3; fn = 4];'
                                  ' iou boxes = 0.75  >>> by area: pr = 0.4667, r = 0.3333, iou = 0.2667, rate = 0.3333')
    with pytest.raises(AssertionError):
        total.get_types_acc()
    c = ev.FtMetrics(["ean", "qr"], True)
    other = ev.FtMetrics(["ean", "qr"], True)
    other.confusion_matrix[:] = [[3, 1], [0.5, 1.5]]
    c.append(other); c.append(other)
    assert np.array_equal(c.confusion_matrix, [[6, 2], [1, 3]])
    assert c.get_average_acc() == 9 / 12
    acc = c.get_types_acc()
    assert acc["ean"] == pytest.approx(6 / 8, abs=1e-5) and acc["qr"] == pytest.approx(3 / 4, abs=1e-5)
    rep = c.get_confusion_matrix_report()
    assert "Average accuracy: 0.750" in rep and "Confusion matrix (predicted \\ actual):" in rep and "0.750" in rep


def test_scalar_logs_key_set():
    thr = ev.DatasetMetricCalculator.IOU_THRESHOLDS
    assert np.array_equal(thr, np.arange(0.4, 1, 0.05)) and len(thr) == 12
    names = ["{:.2f}".format(t) for t in thr]
    assert names == ["0.40", "0.45", "0.50", "0.55", "0.60", "0.65", "0.70", "0.75", "0.80", "0.85", "0.90", "0.95"]
    base = {f"{k}_iou{t}" for t in names for k in ("pr", "recall", "f1", "detection_rate")} | \
        {"average_iou_by_area", "average_precision_by_area", "average_recall_by_area"}
    det = NetConfig(grey=False)
    logs = ev.DatasetMetricCalculator.scalar_logs({t: ev.FtMetrics() for t in thr}, det)
    assert set(logs) == base
    cls = NetConfig(class_names=["ean", "qr"], grey=False)
    logs = ev.DatasetMetricCalculator.scalar_logs({t: ev.FtMetrics(["ean", "qr"], True) for t in thr}, cls)
    assert set(logs) == base | {"types_avg_acc_iou0.50", "acc_ean_iou0.50", "acc_qr_iou0.50"}


def test_ground_truth_is_validated_on_the_host():
    ok = ev.check_ground_truth_polygon([0, 0, 10, 0, 10, 10, 5, 10, 0, 10])                  # a collinear vertex is fine
    assert ok.shape == (5, 2)
    ev.check_ground_truth_polygon([0, 0, 0, 10, 10, 10, 10, 0])                              # clockwise
    with pytest.raises(ValueError, match="image 3, object 1.*not convex"):
        ev.check_ground_truth_polygon([0, 0, 10, 0, 5, 2, 10, 10, 0, 10], 3, 1)               # a reflex corner
    with pytest.raises(ValueError, match="not convex"):
        ev.check_ground_truth_polygon([0, 0, 10, 10, 10, 0, 0, 10])                           # a bow tie
    with pytest.raises(ValueError, match="not convex"):
        ev.check_ground_truth_polygon([0, 3, 10, 3, 2, 9, 5, 0, 8, 9])                        # a pentagram: every turn the same way
    with pytest.raises(ValueError, match="9 vertices"):
        ev.check_ground_truth_polygon([v for a in np.arange(9) * 0.69 for v in (50 * np.cos(a), 50 * np.sin(a))])   # a convex nonagon
    with pytest.raises(ValueError, match="at least 3"):
        ev.check_ground_truth_polygon([0, 0, 1, 1])
    with pytest.raises(ValueError, match="not finite"):
        ev.check_ground_truth_polygon([0, 0, 1, float("nan"), 1, 1])
    with pytest.raises(ValueError, match="image 1"):
        ev.pack_ground_truth([[[0, 0, 1, 0, 1, 1]], []])                                      # evaluation.py:482
    with pytest.raises(ValueError, match="limit is 256"):
        ev.pack_ground_truth([[[0, 0, 1, 0, 1, 1]] * 257])
    with pytest.raises(ValueError, match="image 5, object 1"):
        ev.pack_ground_truth([[[0, 0, 1, 0, 1, 1], [0, 0, 10, 0, 5, 2, 10, 10, 0, 10]]], image_offset=5)
    xy, first, cls, image_first, max_gt = ev.pack_ground_truth([[[0, 0, 1, 0, 1, 1]], [[0, 0, 2, 0, 2, 2, 0, 2], [5, 5, 6, 5, 6, 6]]],
                                                               [[1], [0, 2]])
    assert first.tolist() == [0, 3, 7, 10] and image_first.tolist() == [0, 1, 3] and cls.tolist() == [1, 0, 2] and max_gt == 2
    assert xy.shape == (10, 2) and xy.dtype == np.float64


def test_found_objects_and_type_ids_are_validated_on_the_host():
    """before anything reaches the device (so these run without one): non-convex found quads and type ids out of range"""
    ok = [0, 0, 10, 0, 10, 10, 0, 10]
    for bad, what in (([0, 0, 10, 10, 10, 0, 0, 10], "not convex"), ([0, 0, 10, 0, 2, 2, 0, 10], "not convex"),
                      ([0, 0, 10, 0, 10, 10], "integer coordinates"), ([0, 0, 10.5, 0, 10, 10, 0, 10], "integer coordinates")):
        with pytest.raises(ValueError, match="found object 1 of image 4.*" + what):
            ev.pack_found_objects([[ok, bad]], None, 0, image_offset=4)
    with pytest.raises(ValueError, match="found objects of image 0: object type id 3 is outside 0..2"):
        ev.pack_found_objects([[ok]], [[3]], 3)
    with pytest.raises(ValueError, match="found objects of image 0: object type id -1"):
        ev.pack_found_objects([[ok]], [[-1]], 3)
    with pytest.raises(ValueError, match="ground truth of image 2: object type id 3 is outside 0..2"):
        ev.pack_ground_truth([[ok]], [[3]], image_offset=2, n_classes=3)
    quads, classes, counts = ev.pack_found_objects([[ok, [3, 3, 3, 3, 9, 9, 9, 9]], []], [[1, 0], []], 2)
    assert quads.shape == (2, 2, 8) and counts.tolist() == [2, 0] and classes[0].tolist() == [1, 0] and quads.dtype == np.int32
    # every found quad of the committed batches is valid input of the host-list path (slivers and repeated vertices included)
    for seed, quant in ((ec.SEED_INT, 1), (ec.SEED_QUARTER, 0.25)):
        for g, f in ec.batch(seed, quant, n_random=60):
            assert all(ev._is_convex(np.asarray(q, dtype=np.float64).reshape(4, 2)) for q in f)


def test_no_cpu_path():
    import torch
    from ubdvss_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        ev.FtMetricsCalculator([[0, 0, 10, 0, 10, 10, 0, 10]], [[0, 0, 10, 0, 10, 10, 0, 10]]).analyze(0.5)
    calc = ev.DatasetMetricCalculator(NetConfig(grey=False))
    with pytest.raises(RuntimeError):
        calc.evaluate_batch([[ObjectMarkup([0, 0, 10, 0, 10, 10, 0, 10])]], [[ObjectMarkup([0, 0, 10, 0, 10, 10, 0, 10])]])
    with pytest.raises(RuntimeError):
        calc.get_metrics()
    lib = _lib.load()                                # argument errors are host code: non-zero and a message, here too
    assert lib.ubd_evaluate_accumulator_bytes(12, 3) == (8 + 120 + 108) * 8
    assert lib.ubd_evaluate_workspace_bytes(4, 257, 64, 12, 0) == 0 and lib.ubd_evaluate_workspace_bytes(4, 8, 257, 12, 0) == 0
    assert lib.ubd_evaluate_objects(None, None, None, 1, 4, None, None, 0, None, None, None, 1, None, 1, 0, None, None, None, 0, None) != 0
    assert b"null argument" in lib.ubd_last_error()
