"""GPU: ubd_evaluate_polygons (convex ground truth of up to 64 vertices) against the exact rational oracle of tests/eval_oracle.py,
against ubd_evaluate_objects on common ground, and end to end from a folder of segmentation maps.

Bounds: those of tests/test_gpu_evaluation.py.  Integers exactly (tests/test_evaluation_polygons_host.py asserts that the committed
cases keep every exact IoU 1e-6 clear of 0.05 and of the twelve thresholds); tables and ratios within 1e-9 * max(1, area): the
derivation there gives 1e-11 relative for a boundary sum over 16 edges, so the at most 6 polygons of 64 edges of a union here stay
below 2.4e-10."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import eval_cases as ec  # noqa: E402
import eval_oracle as eo  # noqa: E402
import eval_polygon_cases as pc  # noqa: E402
from ubdvss_amd import NetConfig, Model, ModelRunner, ObjectMarkup, SegmapManager, synthetic, _lib, markup_readers  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

pytestmark = pytest.mark.gpu

THR = ev.DatasetMetricCalculator.IOU_THRESHOLDS
INT_KEYS = ("tp", "fp", "fn", "one_to_one", "one_to_many", "many_to_one", "matched_boxes_count", "detection_rate")
REL = 1e-9
MAXV = _lib.UBD_POLY_MAX_VERTS


@pytest.fixture(scope="module")
def cases():
    """the committed images, their ground truth read on the device (part 1) and required to be the CPU oracle's hulls"""
    maps = np.stack([m for m, _ in pc.images()])
    imgs = pc.batch()
    markup = markup_readers.segmap_polygons(maps)
    for i, (g, _) in enumerate(imgs):
        assert [np.asarray(o.bbox).tolist() for o in markup[i]] == g, i
    return imgs, dict(plain=[eo.Tables([eo.poly(p) for p in g], [eo.poly(p) for p in f]) for g, f in imgs],
                      scaled=[eo.Tables([eo.poly(p) for p in g], [eo.poly(p) for p in f]) for g, f in pc.scaled(imgs)])


def _found_tensors(imgs):
    quads, classes, counts = ev.pack_found_objects([f for _, f in imgs])
    return torch.from_numpy(quads).cuda(), None, torch.from_numpy(counts).cuda()


def _check(imgs, oracles, recs, tabs):
    worst = 0.0
    for i, ((g, f), (ag, af, inter, iou), T) in enumerate(zip(imgs, tabs, oracles)):
        for a in range(len(g)):
            assert abs(ag[a] - float(T.area_g[a])) <= REL * max(1.0, float(T.area_g[a])), (i, a)
            for b in range(len(f)):
                big = max(1.0, float(T.area_g[a]), float(T.area_f[b]))
                e1, e2 = abs(inter[a, b] - float(T.inter[a][b])), abs(iou[a, b] - float(T.iou[a][b]))
                worst = max(worst, e1 / big, e2)
                assert e1 <= REL * big and e2 <= REL, (i, a, b, inter[a, b], float(T.inter[a][b]), iou[a, b], float(T.iou[a][b]))
        for t, thr in enumerate(THR):
            o, r = T.analyze(thr), recs[i, t]
            assert int(r["flags"]) == 0 and int(r["n_gt"]) == len(g) and int(r["n_found"]) == len(f)
            for k in INT_KEYS:
                assert int(r[k]) == o[k], (i, float(thr), k, int(r[k]), o[k])
            assert abs(float(r["iou_sum"]) - float(o["iou_sum"])) <= REL * max(1, o["matched_boxes_count"]), (i, float(thr))
            for k in ("precision_by_area", "recall_by_area", "iou_by_area"):
                worst = max(worst, abs(float(r[k]) - float(o[k])))
                assert abs(float(r[k]) - float(o[k])) <= REL, (i, k, float(r[k]), float(o[k]))
    print(f"polygon evaluation: worst error relative to the bound's scale = {worst:.3e}")


@pytest.mark.parametrize("variant", ["plain", "scaled"])
def test_hull_ground_truth_against_the_exact_oracle(cases, variant):
    imgs, oracles = cases
    quads, classes, counts = _found_tensors(imgs)
    scales = np.array(pc.SCALES, np.float64) if variant == "scaled" else None
    acc = torch.zeros(ev.accumulator_bytes(len(THR), 0), dtype=torch.uint8, device="cuda")
    rec, tables = ev.evaluate_objects(quads, classes, counts, [g for g, _ in imgs], None, THR, 0, acc, scales=scales, return_tables=True)
    tabs = ev.tables_to_numpy(tables, len(imgs), int(quads.shape[1]))
    seen = imgs if variant == "plain" else pc.scaled(imgs)
    _check(seen, oracles[variant], ev.records_to_numpy(rec), tabs)
    kinds = [sum(len(getattr(T, k)) for T in oracles[variant]) for k in ("one_to_ones", "one_to_manys", "many_to_ones")]
    assert all(k >= 1 for k in kinds), kinds
    a = ev.unpack_accumulator(acc.cpu().numpy(), len(THR), 0)
    assert a["images"] == len(imgs) and a["flagged"] == 0


def _raw_polygons(gts, quads, counts, max_verts, per_image=True):
    """ubd_evaluate_polygons itself on host-packed ground truth (no host check of the polygons); returns (rc, records, accumulator)"""
    lib = _lib.load()
    xy = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for g in gts for p in g], axis=0))
    first = np.cumsum([0] + [len(p) // 2 for g in gts for p in g]).astype(np.int32)
    image_first = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
    max_gt = max(len(g) for g in gts)
    n, cap, T = int(quads.shape[0]), int(quads.shape[1]), len(THR)
    thr = np.ascontiguousarray(THR, dtype=np.float64)
    need = int(lib.ubd_evaluate_polygons_workspace_bytes(n, max_gt, cap, T, 0, max_verts))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(ev.accumulator_bytes(T, 0), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((n, T, 80), dtype=torch.uint8, device="cuda")
    xy_d, first_d = torch.from_numpy(xy).cuda(), torch.from_numpy(first).cuda()
    rc = lib.ubd_evaluate_polygons(quads.data_ptr(), None, counts.data_ptr(), n, cap, None, xy_d.data_ptr(), len(xy), first_d.data_ptr(),
                                   None, image_first.ctypes.data, max_gt, thr.ctypes.data, T, 0, max_verts, rec.data_ptr(),
                                   acc.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, ev.records_to_numpy(rec), acc.cpu().numpy()


def test_common_ground_with_the_quad_entry_is_bit_identical():
    imgs = ec.batch(ec.SEED_INT, 1)
    assert max(len(p) // 2 for g, _ in imgs for p in g) <= _lib.UBD_EVAL_MAX_VERTS
    quads, classes, counts = _found_tensors(imgs)
    acc = torch.zeros(ev.accumulator_bytes(len(THR), 0), dtype=torch.uint8, device="cuda")
    rec = ev.evaluate_objects(quads, None, counts, [g for g, _ in imgs], None, THR, 0, acc)       # <= 8 vertices: ubd_evaluate_objects
    rc, rec64, acc64 = _raw_polygons([g for g, _ in imgs], quads, counts, MAXV)
    assert rc == 0, _lib.load().ubd_last_error()
    assert ev.records_to_numpy(rec).tobytes() == rec64.tobytes()
    assert acc.cpu().numpy().tobytes() == acc64.tobytes()
    assert ev.unpack_accumulator(acc64, len(THR), 0)["counters"][:, 0].max() > 0


def test_malformed_polygons_flag_their_image_and_bad_arguments_launch_nothing():
    ang = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    gon65 = np.stack([100 + 80 * np.cos(ang), 100 + 60 * np.sin(ang)], axis=1).reshape(-1).tolist()
    gon64 = np.stack([100 + 80 * np.cos(ang[:64]), 100 + 60 * np.sin(ang[:64])], axis=1).reshape(-1).tolist()
    box = [20, 40, 180, 40, 180, 160, 20, 160]
    gts = [[gon64], [gon65, box], [[1, 1, 9, 9]], [gon64]]
    quads, _, counts = _found_tensors([(None, [box])] * 4)
    rc, recs, acc = _raw_polygons(gts, quads, counts, MAXV)
    assert rc == 0, _lib.load().ubd_last_error()
    assert [int(recs[i, 0]["flags"]) for i in range(4)] == [0, _lib.UBD_EVAL_FLAG_BAD_GT, _lib.UBD_EVAL_FLAG_BAD_GT, 0]
    assert all(int(recs[i, t][k]) == 0 for i in (1, 2) for t in range(len(THR)) for k in INT_KEYS)
    assert recs[0].tobytes() == recs[3].tobytes() and int(recs[0, 0]["tp"]) == 1
    a = ev.unpack_accumulator(acc, len(THR), 0)
    assert a["images"] == 2 and a["flagged"] == 2
    # max_verts below a polygon's size flags it too; outside 3..64 nothing is launched
    rc, recs, _ = _raw_polygons(gts[:1], quads[:1], counts[:1], 32)
    assert rc == 0 and int(recs[0, 0]["flags"]) == _lib.UBD_EVAL_FLAG_BAD_GT
    lib = _lib.load()
    assert lib.ubd_evaluate_polygons_workspace_bytes(1, 1, 1, 12, 0, 65) == 0 and lib.ubd_evaluate_polygons_workspace_bytes(1, 1, 1, 12, 0, 2) == 0
    assert lib.ubd_evaluate_polygons(quads.data_ptr(), None, counts.data_ptr(), 1, 1, None, quads.data_ptr(), 4, quads.data_ptr(), None,
                                     np.zeros(2, np.int32).ctypes.data, 1, np.zeros(1).ctypes.data, 1, 0, 65, None, quads.data_ptr(),
                                     quads.data_ptr(), 1 << 20, None) != 0
    assert b"max_verts" in lib.ubd_last_error()
    # the host path refuses the same polygons by name
    with pytest.raises(ValueError, match="image 1, object 0: 65 vertices, the limit is 64"):
        ev.evaluate_objects(quads, None, counts, gts, None, THR, 0, torch.zeros(ev.accumulator_bytes(len(THR), 0), dtype=torch.uint8, device="cuda"))


def _oracle_logs(gts, founds, cfg):
    ref = {thr: ev.FtMetrics(None, False) for thr in THR}
    for g, f in zip(gts, founds):
        T = eo.Tables([eo.poly(p) for p in g], [eo.poly(p) for p in f])
        for v in T.decision_values():
            assert all(abs(v - Fraction(t)) > Fraction(1, 10 ** 9) for t in [0.05] + [float(x) for x in THR])
        for thr in THR:
            o = T.analyze(thr)
            m = ev.FtMetrics(None, False)
            for k in INT_KEYS[:7]:
                setattr(m, k, o[k])
            m.detection_rate = o["detection_rate"]
            m.average_iou = float(o["iou_sum"]) / o["matched_boxes_count"] if o["matched_boxes_count"] else 0
            m.average_precision_by_area, m.average_recall_by_area, m.average_iou_by_area = (
                float(o["precision_by_area"]), float(o["recall_by_area"]), float(o["iou_by_area"]))
            m.matched_images_count = 1
            ref[thr].append(m)
    return ev.DatasetMetricCalculator.scalar_logs(ref, cfg)


def test_from_a_folder_of_segmentation_maps_to_the_scalar_logs(tmp_path, cases):
    """SegmentationMapMarkupReader on four PNG pairs -> DatasetMetricCalculator over the committed found quads, and ModelRunner.run
    over the images: both give the oracle's scalar logs"""
    imgs, _ = cases
    os.makedirs(tmp_path / "Image")
    os.makedirs(tmp_path / "Detection")
    names = ["img0", "img1", "img2", "img3"]
    pictures = synthetic.textured_images(5, np.stack([q for _, q in pc.images()[:4]]).astype(np.int32), pc.SCALE, 3)
    assert pictures.shape == (4, pc.H, pc.W, 3)
    for k, name in enumerate(names):
        Image.fromarray(pictures[k]).save(tmp_path / "Image" / f"{name}.png")
        Image.fromarray(pc.images()[k][0]).save(tmp_path / "Detection" / f"{name}.png")
    cfg = NetConfig(grey=False)
    reader = markup_readers.SegmentationMapMarkupReader(str(tmp_path), cfg)
    reader.read_markup()
    assert sorted(reader.get_list_of_images()) == names
    gt_objs = [reader.get_image_markup(name) for name in names]
    gts = [[np.asarray(o.bbox).tolist() for o in objs] for objs in gt_objs]
    assert gts == [g for g, _ in imgs[:4]] and max(len(p) // 2 for g in gts for p in g) > _lib.UBD_EVAL_MAX_VERTS
    assert np.array_equal(np.asarray(reader.get_image("img2")), pictures[2])
    calc = ev.DatasetMetricCalculator(cfg)
    calc.evaluate_batch(gt_objs[:3], [[ObjectMarkup(q) for q in f] for _, f in imgs[:3]])
    calc.evaluate_batch(gt_objs[3:], [[ObjectMarkup(q) for q in f] for _, f in imgs[3:4]])
    logs, want = calc.get_metrics(), _oracle_logs(gts, [f for _, f in imgs[:4]], cfg)
    assert sorted(logs) == sorted(want) and want["recall_iou0.50"] > 0
    for k in want:
        assert abs(float(logs[k]) - float(want[k])) <= 1e-9, (k, logs[k], want[k])
    # the device loop over the pictures themselves
    model = Model(cfg, seed=0)
    x = np.stack([np.asarray(reader.get_image(name)) for name in names])
    labels = SegmapManager.build_segmentation_maps_on_device((pc.W, pc.H), gt_objs, scale=pc.SCALE)      # polygon markup: drawn for the overlay
    out, drawn = ModelRunner(cfg).run(model, [(x[:2], gt_objs[:2], None, labels[:2]), (x[2:], gt_objs[2:], None, labels[2:])], 4,
                                      rng=np.random.default_rng(0))
    assert tuple(drawn["gt"].shape) == (2, pc.H, pc.W, 3)
    _, _, found = ModelRunner(cfg).predict(model, x)
    want = _oracle_logs(gts, [[np.asarray(o.bbox).tolist() for o in objs] for objs in found], cfg)
    assert sorted(out) == sorted(want)
    for k in want:
        assert abs(float(out[k]) - float(want[k])) <= 1e-9, (k, out[k], want[k])
