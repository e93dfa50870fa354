"""CPU: the host side of the detection scores and the average precision -- the fp64 AP formula against a brute-force restatement,
the new entry points in the binding, their refusals (checked before the first HIP call, so they answer without a GPU), and the
log keys of a calculator made without the flag."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_oracle as so  # noqa: E402
from ubdvss_amd import NetConfig, _lib  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ubd_score_objects": 11, "ubd_rank_buffer_bytes": 1, "ubd_rank_detections": 12}


def _ap_lists():
    rng = np.random.default_rng(41)
    lists = []
    for k in (2, 3, 7, 40, 200):                                   # random lists
        for _ in range(4):
            tp = rng.random(k) < rng.uniform(0.2, 0.9)
            lists.append((rng.random(k).astype(np.float32), tp, int(tp.sum()) + int(rng.integers(0, 2))))
    lists.append((rng.random(9), np.ones(9, bool), 9))             # all true positives
    lists.append((rng.random(9), np.zeros(9, bool), 4))            # all false positives
    lists.append((np.array([0.3]), np.array([True]), 1))           # single records
    lists.append((np.array([0.3]), np.array([False]), 1))
    lists.append((np.array([0.3]), np.array([True]), 5))
    tied = rng.integers(0, 3, 30) / 4.0                            # tied scores across the list: record order decides
    lists.append((tied, rng.random(30) < 0.5, 30))
    lists.append((np.full(12, 0.5), rng.random(12) < 0.5, 12))
    tp = rng.random(50) < 0.4                                      # far more ground truth than true positives
    lists.append((rng.random(50), tp, int(tp.sum()) + 100))
    with_nan = rng.random(10)
    with_nan[[2, 7]] = np.nan                                      # NaN scores rank last, in record order
    lists.append((with_nan, rng.random(10) < 0.6, 10))
    return [(s, t, max(g, 1)) for s, t, g in lists]


def test_average_precision_equals_the_brute_force_restatement():
    """both are the same fp64 formula; 1e-12 only absorbs the order of the summation"""
    worst = 0.0
    for s, tp, n_gt in _ap_lists():
        got, want = ev.average_precision(s, tp, n_gt), so.average_precision_brute(s, tp, n_gt)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-12, (got, want, len(s), n_gt)
        assert 0.0 <= got <= 1.0 + 1e-12
    assert ev.average_precision([0.9, 0.8, 0.7], [1, 1, 1], 3) == 1.0
    assert ev.average_precision([0.9, 0.8], [0, 0], 3) == 0.0
    assert ev.average_precision([], [], 3) == 0.0
    assert ev.average_precision([0.9, 0.8, 0.7, 0.6], [1, 0, 1, 0], 4) == pytest.approx(0.25 * 1.0 + 0.25 * (2 / 3), abs=1e-15)
    # ties keep record order: the same flags the other way round give another value
    assert ev.average_precision([0.5, 0.5], [1, 0], 1) == 1.0 and ev.average_precision([0.5, 0.5], [0, 1], 1) == 0.5
    for bad in (0, -3):
        with pytest.raises(ValueError):
            ev.average_precision([0.5], [1], bad)


def _header_argument_counts():
    src = open(os.path.join(ROOT, "include", "ubd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(ubd_[a-z_]+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_new_entry_points_are_bound_with_the_headers_argument_counts():
    declared = _header_argument_counts()
    lib = _lib.load()
    for name, count in NEW.items():
        assert declared.get(name) == count, (name, declared.get(name))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == count, name
        assert hasattr(lib, name)
    assert _lib.SIGNATURES["ubd_rank_buffer_bytes"][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 3 and lib.ubd_abi_version() == 3


def test_rank_buffer_bytes():
    lib = _lib.load()
    assert lib.ubd_rank_buffer_bytes(0) == 0 and lib.ubd_rank_buffer_bytes(-5) == 0
    assert lib.ubd_rank_buffer_bytes(1) == 72 and lib.ubd_rank_buffer_bytes(1 << 20) == 64 + 8 * (1 << 20)
    assert ev.rank_buffer_bytes(0) == 0 and ev.rank_buffer_bytes(3) == 88


def test_score_objects_refuses_bad_arguments_before_any_hip_call():
    """host addresses stand in for the device pointers: every case is refused by the argument checks, nothing is launched"""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(logits=p, pixel_stride=1, quads=p, counts=p, n=1, map_h=8, map_w=8, cap=4, scale=4, scores=p)

    def call(**change):
        a = dict(good, **change)
        return lib.ubd_score_objects(a["logits"], a["pixel_stride"], a["quads"], a["counts"], a["n"], a["map_h"], a["map_w"], a["cap"],
                                     a["scale"], a["scores"], None)
    for name in ("logits", "quads", "counts", "scores"):
        assert call(**{name: None}) != 0 and b"ubd_score_objects: null" in lib.ubd_last_error(), name
    for name in ("n", "map_h", "map_w", "cap", "scale", "pixel_stride"):
        for bad in (0, -1):
            assert call(**{name: bad}) != 0 and b"must be positive" in lib.ubd_last_error(), name
    assert call(map_h=32768) != 0 and b"below 32768" in lib.ubd_last_error()
    assert call(map_w=32768) != 0 and b"below 32768" in lib.ubd_last_error()
    assert call(n=3, map_h=32767, map_w=32767) != 0 and b"2^31" in lib.ubd_last_error()
    assert call(n=1 << 15, map_h=256, map_w=256) != 0 and b"2^31" in lib.ubd_last_error()


def test_rank_detections_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    thr = (ctypes.c_double * 16)(*([0.5] * 16))
    good = dict(scores=p, counts=p, n=1, cap=4, iou=p, stride=16, gt_counts=p, thresholds=ctypes.addressof(thr), n_thr=2, buffer=p, capacity=4)

    def call(**change):
        a = dict(good, **change)
        return lib.ubd_rank_detections(a["scores"], a["counts"], a["n"], a["cap"], a["iou"], a["stride"], a["gt_counts"], a["thresholds"],
                                       a["n_thr"], a["buffer"], a["capacity"], None)
    for name in ("scores", "counts", "iou", "gt_counts", "thresholds", "buffer"):
        assert call(**{name: None}) != 0 and b"ubd_rank_detections: null" in lib.ubd_last_error(), name
    assert call(n=0) != 0 and b"n must be positive" in lib.ubd_last_error()
    for bad in (0, -1, _lib.UBD_EVAL_MAX_FOUND + 1):
        assert call(cap=bad) != 0 and b"cap must be 1..256" in lib.ubd_last_error()
    for bad in (0, -1, _lib.UBD_EVAL_MAX_THRESHOLDS + 1):
        assert call(n_thr=bad) != 0 and b"n_thresholds must be 1..16" in lib.ubd_last_error()
    assert call(stride=0) != 0 and b"image_stride_doubles" in lib.ubd_last_error()
    for bad in (0, -7):
        assert call(capacity=bad) != 0 and b"capacity" in lib.ubd_last_error()


def test_log_keys_without_the_flag_are_the_old_ones():
    cfg = NetConfig(class_names=["a", "b"], grey=False)
    thresholds = ev.DatasetMetricCalculator.IOU_THRESHOLDS
    per_iou = {}
    for thr in thresholds:
        m = ev.FtMetrics(["a", "b"], True)
        m.tp, m.fp, m.fn = 3, 1, 2
        per_iou[thr] = m
    want = []
    for thr in thresholds:
        tag = "_iou{:.2f}".format(thr)
        want += [k + tag for k in ("pr", "recall", "f1", "detection_rate")]
        if math.isclose(thr, 0.5):
            want += ["types_avg_acc" + tag, "acc_a" + tag, "acc_b" + tag]
    want += ["average_iou_by_area", "average_precision_by_area", "average_recall_by_area"]
    assert list(ev.DatasetMetricCalculator.scalar_logs(per_iou, cfg)) == want
    assert not [k for k in want if k.startswith("ap_") or k == "map"]
    # the flag is off by default, and a calculator made with it asks for the scores before it touches a device
    plain = ev.DatasetMetricCalculator(cfg, average_precision=False)
    with pytest.raises(RuntimeError, match="without average_precision"):
        plain.get_average_precision()
    with_ap = ev.DatasetMetricCalculator(cfg, average_precision=True, rank_capacity=16)
    with pytest.raises(ValueError, match="scores"):
        with_ap.evaluate_batch([[object()]], [[object()]])
    with pytest.raises(ValueError):
        ev.DatasetMetricCalculator(cfg, average_precision=True, rank_capacity=0)
