"""CPU: the oracle of the pixel classification accuracy (tests/pixel_eval_oracle.py) and the host side of the feature.

The two restatements of the object rule -- border following + contour fill (oracle.cv_post) and labelling + externality
test + hole filling (scipy.ndimage) -- must give the same (correct, size) list on every seeded case, and the numbers
written out for the hand-built quirk maps; the device is checked against the first one in tests/test_gpu_evaluation_pixels.py.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import pixel_eval_oracle as po  # noqa: E402
from ubdvss_amd import NetConfig, _lib  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402


@pytest.mark.parametrize("seed,n,h,w,C", po.seeded_cases())
def test_two_restatements_agree(seed, n, h, w, C):
    labels, z = po.random_batch(seed, n, h, w, C)
    a = po.batch_stats(z[..., 1:], labels, po.objects_contours)
    b = po.batch_stats(z[..., 1:], labels, po.objects_labelling)
    for ia, ib in zip(a, b):
        assert ia["objects"] == ib["objects"]
        assert (ia["n_correct"], ia["n_total"]) == (ib["n_correct"], ib["n_total"])
        assert sum(s for _, s in ia["objects"]) >= ia["n_total"] or not ia["objects"]     # regions cover the foreground


def test_seeded_cases_are_not_trivial():
    """the committed set holds holes, nested components, single pixels and both right and wrong pixels"""
    objs, partly = 0, 0
    for seed, n, h, w, C in po.seeded_cases():
        if h * w < 50 * 70:
            continue
        labels, z = po.random_batch(seed, n, h, w, C)
        for s in po.batch_stats(z[..., 1:], labels):
            objs += len(s["objects"])
            partly += sum(1 for c, sz in s["objects"] if 0 < c < sz)
            assert 0 < s["n_correct"] <= s["n_total"]
            assert C == 1 or s["n_correct"] < s["n_total"]               # one class: every foreground pixel is right
    assert objs > 500 and partly > 100


@pytest.mark.parametrize("name", sorted(po.quirk_maps()))
def test_quirk_maps(name):
    labels, pred, want = po.quirk_maps()[name]
    z = po.logits_from_pred(pred)
    for objects in (po.objects_contours, po.objects_labelling):
        got = po.image_stats(z[..., 1:], labels, objects)
        assert got["n_correct"] == want["n_correct"] and got["n_total"] == want["n_total"]
        assert got["objects"] == want["objects"]
        assert np.array_equal(got["mask"] != 0, labels > 0)


def test_argmax_rule_of_the_oracle():
    z = np.array([[[1.0, 1.0, 0.0], [0.0, np.nan, np.nan], [np.nan, 5.0, 5.0], [0.0, 2.0, 2.0]]], np.float32)
    mask, correct = po.classify(z, np.array([[1, 2, 1, 3]]))
    assert mask.all() and correct.tolist() == [[True, True, True, False]]    # first maximum, first NaN; the second of two equal maxima never wins


def test_pixel_logs_from_sums():
    logs = ev.pixel_logs_from_sums(30, 40, 4, 2.5)
    assert logs == {"classification_pixel_acc_total": 0.75, "classification_pixel_acc_object": 0.625}
    logs = ev.pixel_logs_from_sums(0, 0, 0, 0.0)
    assert set(logs) == {"classification_pixel_acc_total", "classification_pixel_acc_object"}
    assert all(math.isnan(v) for v in logs.values())
    logs = ev.pixel_logs_from_sums(0, 5, 0, 0.0)
    assert logs["classification_pixel_acc_total"] == 0.0 and math.isnan(logs["classification_pixel_acc_object"])


def test_unpack_pixel_accumulator():
    raw = np.zeros(8, np.int64)
    raw[:3] = (7, 9, 2)
    raw[4] = 5
    raw.view(np.float64)[3] = 1.25
    assert ev.unpack_pixel_accumulator(raw.view(np.uint8)) == dict(n_correct=7, n_total=9, n_objects=2, object_acc_sum=1.25, images=5)


def test_new_names_are_bound():
    for name in ("ubd_evaluate_pixels_accumulator_bytes", "ubd_evaluate_pixels_workspace_bytes", "ubd_evaluate_pixels"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ubd_evaluate_pixels"][1]) == 13
    assert _lib.ABI_VERSION == 3
    import ctypes
    assert ctypes.sizeof(_lib.UbdPixelRecord) == 32


def test_header_declares_the_new_entry_points():
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "ubd.h")).read()
    for name in ("ubd_evaluate_pixels_accumulator_bytes", "ubd_evaluate_pixels_workspace_bytes", "ubd_evaluate_pixels(", "ubd_pixel_record"):
        assert name in text


def test_evaluate_batch_without_segmaps_returns_none_mask(monkeypatch):
    cfg = NetConfig(class_names=["a", "b", "c"], grey=False)
    calc = ev.DatasetMetricCalculator(cfg)
    seen = {}

    class _T:
        shape = (1, 4, 8)
        device = "cpu"

        def data_ptr(self):
            return 0

    def fake_objects(quads, classes, counts, polys, cls, thresholds, n_classes, acc, scales=None, image_offset=0):
        seen["called"] = True
        return "records"

    def no_pixels(*a, **k):
        raise AssertionError("the pixel evaluation must not run without label maps and logits")

    monkeypatch.setattr(ev, "_require_gpu", lambda: __import__("torch"))
    monkeypatch.setattr(ev, "evaluate_objects", fake_objects)
    monkeypatch.setattr(ev, "evaluate_pixels", no_pixels)
    monkeypatch.setattr(calc, "_accumulator", lambda device: None)
    from ubdvss_amd import ClassifiedObjectMarkup
    gt = [[ClassifiedObjectMarkup([0, 0, 4, 0, 4, 4, 0, 4], 1)]]
    triple = (_T(), _T(), _T())
    assert calc.evaluate_batch(gt, triple) == ("records", None)
    assert calc.evaluate_batch(gt, triple, gt_segmap=np.zeros((1, 2, 2), np.int32)) == ("records", None)
    assert calc.evaluate_batch(gt, triple, classification_logits=np.zeros((1, 2, 2, 4), np.float32)) == ("records", None)
    assert seen["called"]
    # a detection-only config never scores pixels, whatever it is given
    calc0 = ev.DatasetMetricCalculator(NetConfig(class_names=None, grey=False))
    monkeypatch.setattr(calc0, "_accumulator", lambda device: None)
    from ubdvss_amd import ObjectMarkup
    gt0 = [[ObjectMarkup([0, 0, 4, 0, 4, 4, 0, 4])]]
    assert calc0.evaluate_batch(gt0, triple, gt_segmap=np.zeros((1, 2, 2), np.int32),
                                classification_logits=np.zeros((1, 2, 2, 1), np.float32)) == ("records", None)
