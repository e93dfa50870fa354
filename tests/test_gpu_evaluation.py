"""GPU: ubd_evaluate_objects (areas, IoU tables, 1-1 / 1-many / many-1 matching, group and by-area unions, per-threshold
counters, device sums) against the exact rational oracle of tests/eval_oracle.py.

Bounds.  Tables: absolute error <= 1e-9 * max(1, larger polygon area).  Derived, not measured: coordinates are below 2^14, a
clipped vertex carries a relative error of a few fp64 ulps, a boundary sum over at most 16 edges keeps it below 1e-11 relative;
1e-9 leaves two orders for the union's edge bookkeeping and is four orders tighter than anything a wrong tie rule produces.
The by-area triple and the IoU sums are ratios (<= 1 each) of such areas: the same 1e-9 per ratio.  Confusion weights are
ratios of table entries summed over a handful of objects: 1e-12.  Integer outputs are compared exactly; that is only meaningful
when no exact IoU lies at a threshold, which the committed seeds guarantee and test_inputs_keep_clear_of_every_threshold
asserts with the exact oracle (zero excluded cases).
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import eval_cases as ec  # noqa: E402
import eval_oracle as eo  # noqa: E402
from ubdvss_amd import NetConfig, Model, ModelRunner, ObjectMarkup, ClassifiedObjectMarkup, synthetic, _lib  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

pytestmark = pytest.mark.gpu

THR = ev.DatasetMetricCalculator.IOU_THRESHOLDS
INT_KEYS = ("tp", "fp", "fn", "one_to_one", "one_to_many", "many_to_one", "matched_boxes_count", "detection_rate")
REL = 1e-9


def _device_inputs(imgs, found_cls=None, cap=None):
    cap = cap or max([1] + [len(f) for _, f in imgs])
    n = len(imgs)
    quads = np.zeros((n, cap, 8), np.int32)
    classes = np.zeros((n, cap), np.int32)
    counts = np.zeros(n, np.int32)
    for i, (_, f) in enumerate(imgs):
        counts[i] = len(f)
        for j, q in enumerate(f):
            quads[i, j] = q
        if found_cls is not None:
            classes[i, :len(f)] = found_cls[i]
    return torch.from_numpy(quads).cuda(), torch.from_numpy(classes).cuda(), torch.from_numpy(counts).cuda()


def _evaluate(imgs, thresholds=THR, gt_cls=None, found_cls=None, n_classes=0, scales=None, acc=None, dev_inputs=None):
    quads, classes, counts = dev_inputs if dev_inputs is not None else _device_inputs(imgs, found_cls)
    if acc is None:
        acc = torch.zeros(ev.accumulator_bytes(len(thresholds), n_classes), dtype=torch.uint8, device="cuda")
    rec, tables = ev.evaluate_objects(quads, classes, counts, [g for g, _ in imgs], gt_cls, thresholds, n_classes, acc, scales=scales,
                                      return_tables=True)
    tabs = ev.tables_to_numpy(tables, len(imgs), int(quads.shape[1]))
    return ev.records_to_numpy(rec), tabs, acc


def _oracle_tables(imgs):
    return [eo.Tables([eo.poly(p) for p in g], [eo.poly(p) for p in f]) for g, f in imgs]


def _check_tables(imgs, tabs, oracles):
    worst = 0.0
    for i, ((g, f), (ag, af, inter, iou), T) in enumerate(zip(imgs, tabs, oracles)):
        for a in range(len(g)):
            assert abs(ag[a] - float(T.area_g[a])) <= REL * max(1.0, float(T.area_g[a])), (i, a)
        for b in range(len(f)):
            assert abs(af[b] - float(T.area_f[b])) <= REL * max(1.0, float(T.area_f[b])), (i, b)
        for a in range(len(g)):
            for b in range(len(f)):
                big = max(1.0, float(T.area_g[a]), float(T.area_f[b]))
                e1, e2 = abs(inter[a, b] - float(T.inter[a][b])), abs(iou[a, b] - float(T.iou[a][b]))
                worst = max(worst, e1 / big, e2)
                assert e1 <= REL * big, (i, a, b, inter[a, b], float(T.inter[a][b]))
                assert e2 <= REL, (i, a, b, iou[a, b], float(T.iou[a][b]))
    print(f"tables: worst error relative to the bound's scale = {worst:.3e}")


def _check_records(recs, oracles, thresholds, gt_cls=None, found_cls=None, n_classes=0):
    """every integer exactly, every float to 1e-9; returns the oracle's confusion sums (T, C, C) as Fractions"""
    cm = [[[Fraction(0)] * n_classes for _ in range(n_classes)] for _ in thresholds]
    for i, T in enumerate(oracles):
        for t, thr in enumerate(thresholds):
            o = T.analyze(thr, gt_cls[i] if gt_cls else None, found_cls[i] if found_cls else None, n_classes)
            r = recs[i, t]
            assert int(r["flags"]) == 0 and int(r["n_gt"]) == len(T.gts) and int(r["n_found"]) == len(T.founds)
            for k in INT_KEYS:
                assert int(r[k]) == o[k], (i, float(thr), k, int(r[k]), o[k])
            assert abs(float(r["iou_sum"]) - float(o["iou_sum"])) <= REL * max(1, o["matched_boxes_count"]), (i, float(thr))
            for k in ("precision_by_area", "recall_by_area", "iou_by_area"):
                assert abs(float(r[k]) - float(o[k])) <= REL, (i, k, float(r[k]), float(o[k]))
            for a in range(n_classes):
                for b in range(n_classes):
                    cm[t][a][b] += o["confusion"][a][b]
    return cm


def _assert_clear_of_thresholds(oracles, thresholds=THR):
    """the input condition of the decision checks; zero exclusions are permitted"""
    near = []
    for i, T in enumerate(oracles):
        for v in T.decision_values():
            for t in [0.05] + [float(x) for x in thresholds]:
                if abs(v - Fraction(t)) <= Fraction(1, 10 ** 9):
                    near.append((i, float(v), t))
    assert near == [], near


BATCHES = [("int", ec.SEED_INT, 1), ("quarter", ec.SEED_QUARTER, 0.25)]


@pytest.mark.parametrize("name,seed,quant", BATCHES)
def test_tables_against_exact_areas(name, seed, quant):
    imgs = ec.batch(seed, quant)
    _, tabs, _ = _evaluate(imgs)
    _check_tables(imgs, tabs, _oracle_tables(imgs))


@pytest.mark.parametrize("name,seed,quant", BATCHES)
def test_inputs_keep_clear_of_every_threshold(name, seed, quant):
    _assert_clear_of_thresholds(_oracle_tables(ec.batch(seed, quant)))


@pytest.mark.parametrize("name,seed,quant", BATCHES)
def test_decisions_at_all_twelve_thresholds(name, seed, quant):
    imgs = ec.batch(seed, quant)
    oracles = _oracle_tables(imgs)
    _assert_clear_of_thresholds(oracles)
    recs, _, _ = _evaluate(imgs)
    _check_records(recs, oracles, THR)


def test_decisions_with_three_classes_and_fractional_weights():
    imgs = ec.batch(ec.SEED_INT, 1)
    rng = np.random.default_rng(ec.SEED_CLASSES)
    gt_cls = [[int(c) for c in rng.integers(0, 3, len(g))] for g, _ in imgs]
    found_cls = [[int(c) for c in rng.integers(0, 3, len(f))] for _, f in imgs]
    oracles = _oracle_tables(imgs)
    recs, _, acc = _evaluate(imgs, gt_cls=gt_cls, found_cls=found_cls, n_classes=3)
    cm = _check_records(recs, oracles, THR, gt_cls, found_cls, 3)
    a = ev.unpack_accumulator(acc.cpu().numpy(), len(THR), 3)
    fractional = 0
    for t in range(len(THR)):
        for x in range(3):
            for y in range(3):
                fractional += cm[t][x][y].denominator != 1
                assert abs(a["confusion"][t, x, y] - float(cm[t][x][y])) <= 1e-12 * max(1.0, float(cm[t][x][y])), (t, x, y)
    assert fractional > 0                      # an accepted 1-many with two predicted classes is among the cases


def test_exact_tie_at_a_threshold_follows_the_operators():
    """IoU = 1/2 exactly from integer boxes against the double 0.5: accepted (>=), no detection (strict >)"""
    g, f = ec.tie_image()
    recs, tabs, _ = _evaluate([(g, f)], thresholds=np.array([0.5, 0.5000000001, 0.4999999999]))
    assert tabs[0][3][0, 0] == 0.5
    assert [int(r["tp"]) for r in recs[0]] == [1, 0, 1]
    assert [int(r["detection_rate"]) for r in recs[0]] == [0, 0, 1]


def test_rule_coverage_of_the_committed_seeds():
    for _, seed, quant in BATCHES:
        oracles = _oracle_tables(ec.batch(seed, quant))
        lo = Fraction(float(THR[0]))
        cov = dict(one_to_one_below=sum(1 for T in oracles for m in T.one_to_ones if m[2] < lo),
                   one_to_many_accepted=sum(1 for T in oracles for m in T.one_to_manys if m[2] >= lo),
                   one_to_many_rejected=sum(1 for T in oracles for m in T.one_to_manys if m[2] < lo),
                   many_to_one_accepted=sum(1 for T in oracles for m in T.many_to_ones if m[2] >= lo),
                   many_to_one_rejected=sum(1 for T in oracles for m in T.many_to_ones if m[2] < lo),
                   neither=sum(T.broken_one_to_many for T in oracles),
                   no_found=sum(1 for T in oracles if not T.founds))
        assert all(v >= 1 for v in cov.values()), cov
        # The hand-built images alone satisfy every item above.  The random images are there for breadth of geometry; of the
        # rules they are expected to bring the common ones (1-1 pairs below the lowest threshold, accepted and rejected
        # 1-many groups) and are NOT expected to bring an accepted many-1, a 'neither' or an image without found objects.
        rnd = _oracle_tables(ec.batch(seed, quant, with_listed=False))
        assert sum(1 for T in rnd for m in T.one_to_ones if m[2] < lo) >= 1
        assert sum(1 for T in rnd for m in T.one_to_manys if m[2] >= lo) >= 1
        assert sum(1 for T in rnd for m in T.one_to_manys if m[2] < lo) >= 1


def test_accumulator_is_the_ordered_sum_of_the_records_and_repeats_bit_for_bit():
    imgs = ec.batch(ec.SEED_QUARTER, 0.25)
    parts = [imgs[:9], imgs[9:20], imgs[20:]]

    def run():
        acc = torch.zeros(ev.accumulator_bytes(len(THR), 0), dtype=torch.uint8, device="cuda")
        recs = [_evaluate(p, acc=acc)[0] for p in parts]
        return acc.cpu().numpy().tobytes(), np.concatenate(recs, axis=0)
    b1, recs = run()
    b2, recs2 = run()
    assert b1 == b2 and recs.tobytes() == recs2.tobytes()
    a = ev.unpack_accumulator(np.frombuffer(b1, dtype=np.uint8), len(THR), 0)
    assert a["images"] == len(imgs) and a["flagged"] == 0
    sums = np.zeros(3)
    for i in range(len(imgs)):                                   # image order, one addition per image: the device's order
        sums += [recs[i, 0]["precision_by_area"], recs[i, 0]["recall_by_area"], recs[i, 0]["iou_by_area"]]
    assert sums.tobytes() == a["sums_by_area"].tobytes()
    for t in range(len(THR)):
        s = 0.0
        for i in range(len(imgs)):
            s += recs[i, t]["iou_sum"]
        assert np.float64(s).tobytes() == np.float64(a["iou_sum"][t]).tobytes()
        for c, k in enumerate(INT_KEYS):
            assert int(a["counters"][t, c]) == int(recs[:, t][k].astype(np.int64).sum())


def test_more_than_64_images_in_one_call_equal_the_same_images_in_two_calls():
    """a call walks its images in launches of 64: 70 images (second launch: 6) against the calls 0..32 and 33..69, with classes"""
    imgs = ec.batch(ec.SEED_QUARTER, 0.25, n_random=60)
    assert len(imgs) == 70
    rng = np.random.default_rng(ec.SEED_CLASSES)
    gt_cls = [[int(c) for c in rng.integers(0, 3, len(g))] for g, _ in imgs]
    found_cls = [[int(c) for c in rng.integers(0, 3, len(f))] for _, f in imgs]

    def run(parts):
        acc = torch.zeros(ev.accumulator_bytes(len(THR), 3), dtype=torch.uint8, device="cuda")
        recs, tabs = [], []
        for lo, hi in parts:
            r, t, _ = _evaluate(imgs[lo:hi], gt_cls=gt_cls[lo:hi], found_cls=found_cls[lo:hi], n_classes=3, acc=acc)
            recs.append(r); tabs += t
        return np.concatenate(recs, axis=0), tabs, acc.cpu().numpy()
    r1, t1, a1 = run([(0, 70)])
    r2, t2, a2 = run([(0, 33), (33, 70)])
    assert r1.tobytes() == r2.tobytes() and a1.tobytes() == a2.tobytes()
    for i, (g, f) in enumerate(imgs):                          # the tables too (their strides differ with the call's max_gt and cap)
        assert np.array_equal(t1[i][3][:len(g), :len(f)], t2[i][3][:len(g), :len(f)])
        assert np.array_equal(t1[i][2][:len(g), :len(f)], t2[i][2][:len(g), :len(f)])
    a = ev.unpack_accumulator(a1, len(THR), 3)
    assert a["images"] == 70 and a["flagged"] == 0 and a["counters"][:, 0].max() > 0 and a["confusion"].sum() > 0
    # the images of the second launch against the oracle
    oracles = _oracle_tables(imgs[64:])
    _assert_clear_of_thresholds(oracles)
    _check_records(r1[64:], oracles, THR, gt_cls[64:], found_cls[64:], 3)


def _gt_from_found(quads_h, counts_h, classes_h=None):
    """ground truth made from the found quads read back: every second quad shrunk to 7/8 about its first vertex's opposite
    diagonal centre (dyadic coordinates), the others missed; plus one ground truth far away"""
    gts, gcls = [], []
    for i in range(len(counts_h)):
        g, c = [], []
        for j in range(int(counts_h[i])):
            if j % 3 == 2:
                continue
            q = quads_h[i, j].astype(np.float64).reshape(4, 2)
            ctr = (q[0] + q[2]) / 2
            g.append(list(((q - ctr) * (0.875 if j % 3 == 0 else 0.625) + ctr).reshape(-1)))
            c.append(int((classes_h[i, j] + j) % 3) if classes_h is not None else 0)
        g.append([9000.0, 9000.0, 9040.0, 9000.0, 9040.0, 9030.0])
        c.append(0)
        gts.append(g); gcls.append(c)
    return gts, gcls


def _post_rect_logits(golden_dir, n_cls):
    maps = np.load(os.path.join(golden_dir, "post_rect.npz"))["maps"].astype(np.int32)
    return synthetic.logits_from_maps(maps, n_cls, seed=5, noise=0.0)


@pytest.mark.parametrize("source", ["golden", "synthetic"])
@pytest.mark.parametrize("rescale", [False, True])
def test_postprocess_to_evaluation_without_leaving_the_device(golden_dir, source, rescale):
    n_cls = 3
    lg = _post_rect_logits(golden_dir, n_cls) if source == "golden" else \
        synthetic.logits_from_maps(synthetic.rectangle_maps(31, 6, 128, 128, n_cls), n_cls, seed=8)
    model = Model(NetConfig(class_names=["a", "b", "c"], grey=False), seed=0)
    lt = torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32)).cuda()
    _, quads, classes, counts = model.postprocess_on_device(lt, 0.0, 4, 5, cap=64)
    qh, ch, kh = quads.cpu().numpy(), classes.cpu().numpy(), counts.cpu().numpy()
    assert kh.max() <= 64 and kh.sum() > 0
    n = len(kh)
    scales = np.array([[1.0 + 0.37 * ((i * 7) % 5) / 4, 0.81 + 0.21 * (i % 3)] for i in range(n)]) if rescale else None
    founds = [[(eo.rescale_quad(qh[i, j].tolist(), *scales[i]) if rescale else qh[i, j].tolist()) for j in range(kh[i])] for i in range(n)]
    fq = np.zeros_like(qh)
    for i in range(n):
        for j in range(kh[i]):
            fq[i, j] = founds[i][j]
    gts, gcls = _gt_from_found(fq, kh, ch)
    fcls = [[int(ch[i, j]) for j in range(kh[i])] for i in range(n)]
    imgs = list(zip(gts, founds))
    oracles = _oracle_tables(imgs)
    _assert_clear_of_thresholds(oracles)
    recs, tabs, acc = _evaluate(imgs, gt_cls=gcls, found_cls=fcls, n_classes=n_cls, scales=scales, dev_inputs=(quads, classes, counts))
    _check_tables(imgs, tabs, oracles)
    cm = _check_records(recs, oracles, THR, gcls, fcls, n_cls)
    a = ev.unpack_accumulator(acc.cpu().numpy(), len(THR), n_cls)
    for t in range(len(THR)):
        for x in range(n_cls):
            for y in range(n_cls):
                assert abs(a["confusion"][t, x, y] - float(cm[t][x][y])) <= 1e-12 * max(1.0, float(cm[t][x][y]))


class _Raw:
    """ubd_evaluate_objects with buffers made once (nothing allocated or copied inside the call)"""

    def __init__(self, gts, cap, n_classes=0):
        self.lib = _lib.load()
        xy, first, _, self.image_first, self.max_gt = ev.pack_ground_truth(gts)
        self.nv = len(xy)
        self.xy, self.first = torch.from_numpy(xy).cuda(), torch.from_numpy(first).cuda()
        self.thr = np.ascontiguousarray(THR, dtype=np.float64)
        self.n, self.cap, self.C = len(gts), cap, n_classes
        self.acc = torch.zeros(ev.accumulator_bytes(len(THR), n_classes), dtype=torch.uint8, device="cuda")
        self.need = int(self.lib.ubd_evaluate_workspace_bytes(self.n, self.max_gt, cap, len(THR), n_classes))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")

    def __call__(self, quads, counts, acc=True, image_first=None):
        first = self.image_first if image_first is None else image_first
        return self.lib.ubd_evaluate_objects(
            quads.data_ptr(), None, counts.data_ptr(), self.n, self.cap, None, self.xy.data_ptr(), self.nv, self.first.data_ptr(), None,
            first.ctypes.data, self.max_gt, self.thr.ctypes.data, len(THR), self.C, None, self.acc.data_ptr() if acc else None,
            self.ws.data_ptr(), self.need, torch.cuda.current_stream().cuda_stream)


def test_forward_postprocess_evaluation_in_one_hip_graph():
    cfg = NetConfig(grey=False)
    model = Model(cfg, seed=0)
    labels = synthetic.rectangle_maps(3, 4, 32, 32)
    x = torch.from_numpy(synthetic.textured_images(4, labels, 4, 3)).cuda()
    n, cap = 4, 64
    gts = [[[8.0, 8.0, 60.0, 8.0, 60.0, 40.0, 8.0, 40.0], [70.0, 70.0, 120.0, 70.0, 95.0, 120.0]] for _ in range(n)]
    raw = _Raw(gts, cap)
    logits = torch.empty((n, 32, 32, model.k_out), dtype=torch.float32, device="cuda")
    outs = model.alloc_postprocess_outputs(n, 32, 32, cap)

    def chain(prepacked):
        model.predict_on_device(x, out=logits, _prepacked=prepacked)
        model.postprocess_on_device(logits, -2.0, 4, 5, cap=cap, outputs=outs)
        assert raw(outs[1], outs[3]) == 0, _lib.load().ubd_last_error()
    chain(False); chain(False)
    torch.cuda.synchronize()
    raw.acc.zero_()
    chain(False)
    torch.cuda.synchronize()
    direct = raw.acc.cpu().numpy().tobytes()
    a = ev.unpack_accumulator(np.frombuffer(direct, dtype=np.uint8), len(THR), 0)
    assert a["images"] == n and a["flagged"] == 0
    raw.acc.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(True)
    raw.acc.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert raw.acc.cpu().numpy().tobytes() == direct
    g.replay()                                                   # sums keep adding: twice the integers
    torch.cuda.synchronize()
    b = ev.unpack_accumulator(raw.acc.cpu().numpy(), len(THR), 0)
    assert b["images"] == 2 * n and (b["counters"] == 2 * a["counters"]).all()


def test_overflow_is_flagged_and_bad_arguments_launch_nothing():
    imgs = ec.listed_images()[:4]
    quads, classes, counts = _device_inputs(imgs, cap=4)
    counts[1] = 7                                                # more than cap: the list of image 1 was truncated
    recs, _, acc = _evaluate(imgs, dev_inputs=(quads, classes, counts))
    assert [int(recs[i, 0]["flags"]) for i in range(4)] == [0, _lib.UBD_EVAL_FLAG_OVERFLOW, 0, 0]
    assert all(int(recs[1, t][k]) == 0 for t in range(len(THR)) for k in INT_KEYS)
    a = ev.unpack_accumulator(acc.cpu().numpy(), len(THR), 0)
    assert a["images"] == 3 and a["flagged"] == 1
    calc = ev.DatasetMetricCalculator(NetConfig(grey=False))
    calc.evaluate_batch([[ObjectMarkup(p) for p in g] for g, _ in imgs], (quads, None, counts))
    with pytest.raises(RuntimeError, match="not scored"):
        calc.get_metrics()
    # host object lists are validated before anything is enqueued
    cls_calc = ev.DatasetMetricCalculator(NetConfig(class_names=["a", "b"], grey=False))
    ok = [0, 0, 10, 0, 10, 10, 0, 10]
    with pytest.raises(ValueError, match="not convex"):
        cls_calc.evaluate_batch([[ClassifiedObjectMarkup(ok, 0)]], [[ClassifiedObjectMarkup([0, 0, 10, 10, 10, 0, 0, 10], 0)]])
    with pytest.raises(ValueError, match="type id 2"):
        cls_calc.evaluate_batch([[ClassifiedObjectMarkup(ok, 0)]], [[ClassifiedObjectMarkup(ok, 2)]])
    with pytest.raises(ValueError, match="type id 5"):
        cls_calc.evaluate_batch([[ClassifiedObjectMarkup(ok, 5)]], [[ClassifiedObjectMarkup(ok, 1)]])
    # argument errors: non-zero, a message, and the accumulator untouched
    raw = _Raw([g for g, _ in imgs], 4)
    lib = _lib.load()
    assert raw(quads, counts, acc=False) != 0 and b"accumulator" in lib.ubd_last_error()
    too_many = np.array([0, _lib.UBD_EVAL_MAX_GT + 1, _lib.UBD_EVAL_MAX_GT + 2, _lib.UBD_EVAL_MAX_GT + 3, _lib.UBD_EVAL_MAX_GT + 4], np.int32)
    assert raw(quads, counts, image_first=too_many) != 0 and b"limit is 256" in lib.ubd_last_error()
    torch.cuda.synchronize()
    assert not raw.acc.cpu().numpy().any()
    assert lib.ubd_evaluate_workspace_bytes(4, 300, 4, 12, 0) == 0


def test_dataset_calculator_and_model_runner_give_the_scalar_logs():
    """DatasetMetricCalculator over host object lists = the oracle's sums; ModelRunner.evaluate_batches runs the device loop"""
    imgs = ec.batch(ec.SEED_INT, 1)
    cfg = NetConfig(class_names=["a", "b", "c"], grey=False)
    rng = np.random.default_rng(ec.SEED_CLASSES)
    gt_objs = [[ClassifiedObjectMarkup(p, int(rng.integers(3))) for p in g] for g, _ in imgs]
    f_objs = [[ClassifiedObjectMarkup(q, int(rng.integers(3))) for q in f] for _, f in imgs]
    calc = ev.DatasetMetricCalculator(cfg)
    calc.evaluate_batch(gt_objs[:15], f_objs[:15])
    calc.evaluate_batch(gt_objs[15:], f_objs[15:])
    logs = calc.get_metrics()
    oracles = _oracle_tables(imgs)
    ref = {thr: ev.FtMetrics(["a", "b", "c"], True) for thr in THR}
    for i, T in enumerate(oracles):
        for thr in THR:
            o = T.analyze(thr, [m.object_type for m in gt_objs[i]], [m.object_type for m in f_objs[i]], 3)
            m = ev.FtMetrics(["a", "b", "c"], True)
            for k in INT_KEYS[:7]:
                setattr(m, k, o[k])
            m.detection_rate = o["detection_rate"]
            m.average_iou = float(o["iou_sum"]) / o["matched_boxes_count"] if o["matched_boxes_count"] else 0
            m.average_precision_by_area, m.average_recall_by_area, m.average_iou_by_area = (
                float(o["precision_by_area"]), float(o["recall_by_area"]), float(o["iou_by_area"]))
            m.matched_images_count = 1
            m.confusion_matrix = np.array([[float(v) for v in row] for row in o["confusion"]])
            ref[thr].append(m)
    want = ev.DatasetMetricCalculator.scalar_logs(ref, cfg)
    assert sorted(logs) == sorted(want)
    for k in want:
        assert abs(float(logs[k]) - float(want[k])) <= 1e-9, (k, logs[k], want[k])
    # the device loop: forward -> postprocess -> evaluation, one read at the end
    det_cfg = NetConfig(grey=False)
    model = Model(det_cfg, seed=0)
    labels = synthetic.rectangle_maps(3, 4, 32, 32)
    x = synthetic.textured_images(4, labels, 4, 3)

    class Meta:
        xscale, yscale = 1.5, 0.75
    gt = [[ObjectMarkup([8, 8, 60, 8, 60, 40, 8, 40])] for _ in range(4)]
    runner = ModelRunner(det_cfg)
    out = runner.evaluate_batches(model, [(x[:2], gt[:2], [Meta(), Meta()]), (x[2:], gt[2:], [Meta(), Meta()])])
    _, _, found = ModelRunner(det_cfg).predict(model, x, rescale=True, meta_infos=[Meta()] * 4)
    calc2 = ev.DatasetMetricCalculator(det_cfg)
    calc2.evaluate_batch(gt, found)
    assert out == calc2.get_metrics()
