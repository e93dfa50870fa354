"""MI355X: ubd_score_objects against the fp64 oracle (2e-6 absolute), ubd_rank_detections bit for bit against the numpy matcher,
and the chain postprocess -> score -> evaluate -> rank through Model / ModelRunner / DatasetMetricCalculator, once inside a HIP
graph.  No reference counterpart: the definitions are the project's (include/ubd.h), restated in tests/score_oracle.py."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_oracle as so  # noqa: E402
from ubdvss_amd import NetConfig, Model, ModelRunner, MultiscaleModel, ObjectMarkup, synthetic, _lib  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

pytestmark = pytest.mark.gpu

# 4 ulp of the fp32 sigmoid (expf, add, divide) on a value <= 1 is 2.4e-7; the quantisation and the final rounding add at most
# 2^-24 = 6e-8 together: 2e-6 leaves a margin of about five
SCORE_TOL = 2e-6
THR = ev.DatasetMetricCalculator.IOU_THRESHOLDS


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------- ubd_score_objects
def _box(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def _to_image(quad_map, scale, rng):
    """map coordinates -> image coordinates that snap back to a box at least as large: times scale, plus a jitter below scale"""
    q = np.asarray(quad_map, dtype=np.int64) * scale
    return q + (rng.integers(0, scale, 8) if scale > 1 else 0)


def _logits(rng, n, h, w, stride, special):
    lg = rng.normal(0.0, 3.0, (n, h, w, stride)).astype(np.float32)
    for k, (i, y, x) in enumerate(special):
        if y < h and x < w:
            lg[i, y, x, 0] = (40.0, -40.0, np.nan)[k % 3]
    return lg


def _score(lg, quads, counts, cap, scale):
    """device scores of one call, twice: returns the first after checking that the second has the same bits"""
    lib = _lib.load()
    n, h, w, stride = lg.shape
    lt = torch.from_numpy(lg).cuda()
    qt, ct = torch.from_numpy(quads.astype(np.int32)).cuda(), torch.from_numpy(counts.astype(np.int32)).cuda()
    outs = []
    for fill in (7.0, -3.0):
        out = torch.full((n, cap), fill, dtype=torch.float32, device="cuda")
        rc = lib.ubd_score_objects(lt.data_ptr(), stride, qt.data_ptr(), ct.data_ptr(), n, h, w, cap, scale, out.data_ptr(), _stream())
        assert rc == 0, lib.ubd_last_error()
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def _check_scores(lg, quads, counts, cap, scale):
    got = _score(lg, quads, counts, cap, scale)
    want = so.score_objects(lg[..., 0], quads, counts, scale)
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"ubd_score_objects: largest |device - oracle| = {diff:.3e} on map {lg.shape[1]} x {lg.shape[2]}, stride {lg.shape[3]}, scale {scale}")
    assert diff <= SCORE_TOL, f"largest difference {diff:.3e} > {SCORE_TOL}"
    for i in range(len(counts)):
        assert not got[i, max(min(int(counts[i]), cap), 0):].any(), "slots past the count must be exactly 0.0"
    return got, want


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("scale", [1, 4])
def test_scores_against_the_oracle(stride, scale):
    rng = np.random.default_rng(100 * stride + scale)
    # a 5 x 7 map with a one-pixel quad (and a 2 x 2 one beside it)
    quads = np.zeros((1, 2, 8), np.int64)
    quads[0, 0] = np.asarray(_box(3, 2, 3, 2)) * scale
    quads[0, 1] = np.asarray(_box(5, 3, 6, 4)) * scale
    lg = _logits(rng, 1, 5, 7, stride, [(0, 2, 3)])
    got, want = _check_scores(lg, quads, np.array([2]), 2, scale)
    p = 1.0 / (1.0 + math.exp(-40.0))
    assert want[0, 0] == np.float32(p) and abs(float(got[0, 0]) - p) <= SCORE_TOL       # the one pixel is the +40 one
    # a 9 x 70 map: a box wider than two runs from an odd x, boxes cut by each border, one outside, one rotated by 30 degrees
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    rot = [int(round(v)) for dx, dy in ((-12, -2.5), (12, -2.5), (12, 2.5), (-12, 2.5)) for v in (35 + dx * c - dy * s, 4.5 + dx * s + dy * c)]
    boxes = [_box(3, 2, 69, 5), _box(-4, 1, 3, 3), _box(66, 4, 75, 6), _box(20, -3, 27, 1), _box(40, 7, 47, 12), _box(80, 2, 90, 4),
             _box(10, -9, 14, -5), rot]
    quads = np.stack([_to_image(b, scale, rng) for b in boxes])[None]
    lg = _logits(rng, 1, 9, 70, stride, [(0, 3, 10), (0, 4, 40), (0, 3, 50), (0, 2, 2), (0, 5, 68), (0, 0, 22), (0, 8, 44), (0, 4, 33)])
    got, want = _check_scores(lg, quads, np.array([len(boxes)]), len(boxes), scale)
    assert got[0, 5] == 0.0 and got[0, 6] == 0.0                    # wholly outside: an empty region scores 0
    assert (got[0, [0, 1, 2, 3, 4, 7]] > 0).all()
    assert so.region_mask(quads[0, 0], scale, 9, 70)[3].sum() > 64  # the wide box does span more than two runs of a row
    # n = 3 with counts (0, 2, cap + 1) at cap = 4: an image over its capacity scores its first cap entries
    cap = 4
    quads = rng.integers(-50, 50, (3, cap, 8))                      # what lies behind a list's end is unspecified
    for i, k in ((1, 2), (2, cap)):
        for o in range(k):
            x0, y0 = int(rng.integers(0, 50)), int(rng.integers(0, 6))
            quads[i, o] = _to_image(_box(x0, y0, x0 + int(rng.integers(1, 20)), y0 + int(rng.integers(0, 4))), scale, rng)
    got, want = _check_scores(_logits(rng, 3, 9, 70, stride, [(1, 3, 10), (2, 4, 40), (2, 3, 50)]), quads, np.array([0, 2, cap + 1]), cap, scale)
    assert not got[0].any() and (got[2] > 0).all()


def test_model_scores_its_own_postprocess_through_the_multiscale_forwarding():
    cfg = NetConfig(class_names=["a", "b"], grey=False)
    model = Model(cfg, seed=0)
    lg = synthetic.logits_from_maps(synthetic.rectangle_maps(4, 3, 64, 96, 2), 2, seed=3, noise=1.5)
    lt = torch.from_numpy(lg).cuda()
    _, quads, _, counts = model.postprocess_on_device(lt, 0.0, 4, 5, cap=32)
    got = model.score_objects_on_device(lt, quads, counts, 4)
    again = MultiscaleModel(model, 1).score_objects_on_device(lt, quads, counts, 4)
    assert tuple(got.shape) == (3, 32) and got.dtype == torch.float32 and torch.equal(got, again)
    qh, kh = quads.cpu().numpy(), counts.cpu().numpy()
    assert kh.sum() > 0 and kh.max() <= 32
    want = so.score_objects(lg[..., 0], qh, kh, 4)
    diff = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    assert diff <= SCORE_TOL, f"largest difference {diff:.3e}"
    assert (want[np.arange(32)[None] < kh[:, None]] > 0).all()      # every found box lies on the map


# -------------------------------------------------------------------------------------------------------- ubd_rank_detections
class _Ranker:
    """ubd_rank_detections on host-made inputs uploaded once; iou: (n, rows, cap) float64"""

    def __init__(self, scores, counts, iou, gt_counts, thresholds, capacity, pad=3):
        self.lib = _lib.load()
        self.n, self.cap = scores.shape
        self.h = (scores.astype(np.float32), counts.astype(np.int32), iou.astype(np.float64), gt_counts.astype(np.int32))
        self.thr = np.ascontiguousarray(thresholds, dtype=np.float64)
        self.capacity = capacity
        self.stride = iou.shape[1] * self.cap + pad
        flat = np.full((self.n, self.stride), -7.0)
        flat[:, :iou.shape[1] * self.cap] = iou.reshape(self.n, -1)
        self.d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (self.h[0], self.h[1], flat, self.h[3])]
        self.buf = torch.zeros(ev.rank_buffer_bytes(capacity), dtype=torch.uint8, device="cuda")

    def __call__(self):
        s, c, t, g = self.d
        rc = self.lib.ubd_rank_detections(s.data_ptr(), c.data_ptr(), self.n, self.cap, t.data_ptr(), self.stride, g.data_ptr(),
                                          self.thr.ctypes.data, len(self.thr), self.buf.data_ptr(), self.capacity, _stream())
        assert rc == 0, self.lib.ubd_last_error()

    def add_to(self, oracle):
        s, c, iou, g = self.h
        oracle.add(s, c, self.cap, iou, g, self.thr)

    def bytes(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy().tobytes()


def _sixteen_thresholds():
    thr = np.array([0.05 * k for k in range(4, 20)])
    thr[6] = 0.5
    return thr


def _small_case():
    """n = 3, cap = 5, ground truths (1, 3, 0): equal scores, equal IoUs in a column, an IoU equal to a threshold, NaNs"""
    scores = np.array([[0.9, 0.9, 0.2, 0.9, 0.0],                  # equal scores: the lower index goes first
                       [0.3, np.nan, 0.8, 0.3, 0.6],               # a NaN score ranks last
                       [0.5, 0.1, 0.7, 0.0, 0.0]], np.float32)
    counts = np.array([4, 5, 3])
    iou = np.zeros((3, 3, 5))
    iou[0, 0] = [0.5, 0.9, 0.3, 0.5, 0.99]                         # 0.5 exactly at the threshold 0.5; slot 4 lies behind the list
    iou[1] = [[0.6, 0.7, 0.6, 0.2, np.nan],                        # column 2: equal IoUs with two ground truths -> the lowest g
              [0.6, 0.8, 0.6, 0.75, 0.45],
              [0.1, np.nan, 0.25, 0.75, 0.45]]                     # column 3: equal again; column 4: a NaN never matches
    iou[2] = 0.9                                                   # no ground truth: every detection is a false positive
    return scores, counts, iou, np.array([1, 3, 0])


@pytest.mark.parametrize("thresholds", [_sixteen_thresholds(), np.array([0.5])], ids=["16", "1"])
def test_rank_small_case_bit_for_bit(thresholds):
    r = _Ranker(*_small_case(), thresholds, 64)
    r()
    oracle = so.RankBuffer(64)
    r.add_to(oracle)
    first = r.bytes()
    assert first == oracle.tobytes()
    u = ev.unpack_rank_buffer(np.frombuffer(first, np.uint8))
    assert (u["written"], u["dropped"], u["n_gt"], u["images"], u["flagged"]) == (12, 0, 4, 3, 0)
    assert np.isnan(u["scores"][8]) and not u["tp_mask"][9:].any()
    j = int(np.flatnonzero(thresholds == 0.5)[0])
    assert (u["tp_mask"][0] >> j) & 1                               # 0.9 with IoU 0.5: accepted at the threshold 0.5 (>=)
    # a second call appends: the concatenation, and the same bytes when everything is done again
    r()
    r.add_to(oracle)
    both = r.bytes()
    assert both == oracle.tobytes() and both[64:64 + 12 * 8] == first[64:64 + 12 * 8]
    r.buf.zero_()
    r(); r()
    assert r.bytes() == both


def test_rank_at_the_limits_of_256_found_and_256_ground_truths():
    rng = np.random.default_rng(9)
    scores = (rng.integers(0, 40, (1, 256)) / 40.0).astype(np.float32)          # many equal scores
    iou = np.round(rng.random((1, 256, 256)) ** 3, 2)                           # many equal IoUs, some at a threshold
    r = _Ranker(scores, np.array([256]), iou, np.array([256]), _sixteen_thresholds(), 300)
    r()
    oracle = so.RankBuffer(300)
    r.add_to(oracle)
    assert r.bytes() == oracle.tobytes()
    u = ev.unpack_rank_buffer(np.frombuffer(r.bytes(), np.uint8))
    assert u["written"] == 256 and u["n_gt"] == 256 and 0 < int((u["tp_mask"] & 1).sum()) <= 256


def test_rank_flags_an_overflowing_image_and_counts_dropped_records():
    scores, counts, iou, gt = _small_case()
    counts = counts.copy()
    counts[0] = 6                                                   # more than cap = 5: the list was truncated
    gt2 = np.array([1, 3, 257])                                     # more ground truth than a table holds
    r = _Ranker(scores, counts, iou, gt, THR, 64)
    r()
    oracle = so.RankBuffer(64)
    r.add_to(oracle)
    assert r.bytes() == oracle.tobytes()
    u = ev.unpack_rank_buffer(np.frombuffer(r.bytes(), np.uint8))
    assert (u["written"], u["n_gt"], u["images"], u["flagged"]) == (8, 3, 2, 1)
    r = _Ranker(scores, _small_case()[1], iou, gt2, THR, 64)
    r()
    u = ev.unpack_rank_buffer(np.frombuffer(r.bytes(), np.uint8))
    assert (u["written"], u["n_gt"], u["images"], u["flagged"]) == (9, 4, 2, 1)
    # capacity 7 for 12 records: the first 7 are intact, 5 are counted as dropped; a further call drops all of its 12
    r = _Ranker(*_small_case(), THR, 7)
    full = _Ranker(*_small_case(), THR, 64)
    r(); full()
    oracle = so.RankBuffer(7)
    r.add_to(oracle)
    assert r.bytes() == oracle.tobytes() and r.bytes()[64:] == full.bytes()[64:64 + 7 * 8]
    u = ev.unpack_rank_buffer(np.frombuffer(r.bytes(), np.uint8))
    assert (u["written"], u["dropped"], u["n_gt"], u["images"]) == (7, 5, 4, 3)
    r()
    r.add_to(oracle)
    assert r.bytes() == oracle.tobytes()
    assert ev.unpack_rank_buffer(np.frombuffer(r.bytes(), np.uint8))["dropped"] == 17


# ------------------------------------------------------------------------------------------------------------------- the chain
def _gt_from_found(quads_h, counts_h):
    """ground truth from the found quads read back: two of three shrunk about their centre, the third missed, one far away"""
    gts = []
    for i in range(len(counts_h)):
        g = []
        for j in range(int(counts_h[i])):
            if j % 3 == 2:
                continue
            q = quads_h[i, j].astype(np.float64).reshape(4, 2)
            ctr = (q[0] + q[2]) / 2
            g.append(list(((q - ctr) * (0.875 if j % 3 == 0 else 0.625) + ctr).reshape(-1)))
        g.append([9000.0, 9000.0, 9040.0, 9000.0, 9040.0, 9030.0])
        gts.append(g)
    return gts


def _oracle_records(scores_h, counts_h, cap, tables_h, gts, capacity):
    oracle = so.RankBuffer(capacity)
    oracle.add(scores_h, counts_h, cap, [t[3] for t in tables_h], np.array([len(g) for g in gts]), THR)
    return oracle


def test_chain_postprocess_score_evaluate_rank_on_the_device():
    cfg = NetConfig(grey=False)
    model = Model(cfg, seed=0)
    lg = synthetic.logits_from_maps(synthetic.rectangle_maps(31, 6, 128, 128), 0, seed=8, noise=1.5)
    lt = torch.from_numpy(lg).cuda()
    cap = 64
    _, quads, _, counts = model.postprocess_on_device(lt, 0.0, 4, 5, cap=cap)
    scores = model.score_objects_on_device(lt, quads, counts, 4)
    qh, kh = quads.cpu().numpy(), counts.cpu().numpy()
    assert kh.max() <= cap and kh.sum() > 6
    gts = _gt_from_found(qh, kh)
    acc = torch.zeros(ev.accumulator_bytes(len(THR), 0), dtype=torch.uint8, device="cuda")
    _, tables = ev.evaluate_objects(quads, None, counts, gts, None, THR, 0, acc, return_tables=True)
    buf = torch.zeros(ev.rank_buffer_bytes(1024), dtype=torch.uint8, device="cuda")
    ev.rank_detections(scores, counts, gts, tables, THR, buf)
    torch.cuda.synchronize()
    # exact: the numpy matcher on the device's own scores and IoU tables
    sh, th = scores.cpu().numpy(), ev.tables_to_numpy(tables, len(kh), cap)
    oracle = _oracle_records(sh, kh, cap, th, gts, 1024)
    assert buf.cpu().numpy().tobytes() == oracle.tobytes()
    u = ev.unpack_rank_buffer(buf.cpu().numpy())
    assert u["written"] == int(kh.sum()) and u["n_gt"] == sum(len(g) for g in gts) and u["flagged"] == 0
    assert len(set(u["scores"].tolist())) > 3 and u["tp_mask"].any()
    # the calculator: the same records, and the AP of exactly those records
    gt_objs = [[ObjectMarkup(p) for p in g] for g in gts]
    calc = ev.DatasetMetricCalculator(cfg, average_precision=True, rank_capacity=1024)
    plain = ev.DatasetMetricCalculator(cfg)
    for a, b in ((0, 2), (2, 6)):
        calc.evaluate_batch(gt_objs[a:b], (quads[a:b], None, counts[a:b]), scores=scores[a:b])
        plain.evaluate_batch(gt_objs[a:b], (quads[a:b], None, counts[a:b]))
    ap = calc.get_average_precision()
    assert list(ap) == ["ap_iou{:.2f}".format(t) for t in THR] + ["map"]
    for j, t in enumerate(THR):
        assert ap["ap_iou{:.2f}".format(t)] == ev.average_precision(u["scores"], (u["tp_mask"] >> j) & 1, u["n_gt"])
    assert ap["map"] == float(np.mean([ap["ap_iou{:.2f}".format(t)] for t in THR])) and 0 < ap["map"] <= 1
    assert ap["ap_iou0.40"] >= ap["ap_iou0.95"]
    old, new = plain.get_metrics(), calc.get_metrics()
    assert {k: v for k, v in new.items() if k not in ap} == old and all(new[k] == ap[k] for k in ap)
    # scores as host lists beside host object lists give the same records
    host = ev.DatasetMetricCalculator(cfg, average_precision=True, rank_capacity=1024)
    host.evaluate_batch(gt_objs, [[ObjectMarkup(qh[i, j]) for j in range(kh[i])] for i in range(len(kh))],
                        scores=[sh[i, :kh[i]] for i in range(len(kh))])
    assert host.get_average_precision() == ap
    # too small a buffer is reported, not averaged
    tight = ev.DatasetMetricCalculator(cfg, average_precision=True, rank_capacity=3)
    tight.evaluate_batch(gt_objs, (quads, None, counts), scores=scores)
    with pytest.raises(RuntimeError, match="dropped"):
        tight.get_average_precision()


def test_model_runner_opt_in_keeps_the_old_keys_and_values():
    cfg = NetConfig(grey=False)
    model = Model(cfg, seed=0)
    labels = synthetic.rectangle_maps(3, 4, 32, 32)
    x = synthetic.textured_images(4, labels, 4, 3)

    class Meta:
        xscale, yscale = 1.5, 0.75
    gt = [[ObjectMarkup([8, 8, 60, 8, 60, 40, 8, 40])] for _ in range(4)]
    batches = [(x[:2], gt[:2], [Meta(), Meta()]), (x[2:], gt[2:], [Meta(), Meta()])]
    runner = ModelRunner(cfg, pixel_threshold=0.12)                 # a low threshold: untrained weights find objects
    off = runner.evaluate_batches(model, batches)
    on = runner.evaluate_batches(model, batches, average_precision=True)
    keys = ["ap_iou{:.2f}".format(t) for t in THR] + ["map"]
    assert not [k for k in off if k.startswith("ap_") or k == "map"]
    assert {k: v for k, v in on.items() if k not in keys} == off and sorted(set(on) - set(off)) == sorted(keys)
    # flag off: exactly what the calculator gives for predict's objects, as before
    det, cls_logits, found = ModelRunner(cfg, pixel_threshold=0.12).predict(model, x, rescale=True, meta_infos=[Meta()] * 4)
    calc = ev.DatasetMetricCalculator(cfg)
    calc.evaluate_batch(gt, found)
    assert off == calc.get_metrics()
    with_maps = [(x[:2], gt[:2], [Meta(), Meta()], labels[:2]), (x[2:], gt[2:], [Meta(), Meta()], labels[2:])]
    run_logs, _ = runner.run(model, with_maps, 4, rng=np.random.default_rng(0), average_precision=True)
    assert run_logs == on
    # predict_scored: predict's triple, the scores beside the records, min_score on the host; a pipelined runner is flushed
    for piped in (False, True):
        r = ModelRunner(cfg, pixel_threshold=0.12, pipelined=piped)
        det2, cls2, found2, scores = r.predict_scored(model, x, rescale=True, meta_infos=[Meta()] * 4)
        assert np.array_equal(det2, det) and np.array_equal(cls2, cls_logits)
        assert [[list(o.bbox) for o in f] for f in found2] == [[list(o.bbox) for o in f] for f in found]
        assert [len(s) for s in scores] == [len(f) for f in found] and all(s.dtype == np.float32 for s in scores)
        flat = np.concatenate(scores)
        assert len(flat) > 0 and ((flat >= 0) & (flat <= 1)).all()   # the low threshold makes the untrained net find objects
        cut = float(np.median(flat))
        _, _, kept, kept_scores = r.predict_scored(model, x, min_score=cut)
        assert [len(k) for k in kept] == [int((s >= cut).sum()) for s in scores]
        assert all((s >= cut).all() for s in kept_scores)


def _capturing_graph_shape():
    """(nodes, [(from, to)], dependencies of the next node) of the graph the current stream is capturing, from the HIP runtime"""
    hip = ctypes.CDLL("libamdhip64.so")
    status, ident, graph = ctypes.c_int(), ctypes.c_ulonglong(), ctypes.c_void_p()
    deps, n_deps = ctypes.c_void_p(), ctypes.c_size_t()
    assert hip.hipStreamGetCaptureInfo_v2(ctypes.c_void_p(_stream()), ctypes.byref(status), ctypes.byref(ident), ctypes.byref(graph),
                                          ctypes.byref(deps), ctypes.byref(n_deps)) == 0
    assert status.value == 1 and graph.value                        # hipStreamCaptureStatusActive
    n_nodes, n_edges = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n_edges)) == 0
    src, dst = (ctypes.c_void_p * max(n_edges.value, 1))(), (ctypes.c_void_p * max(n_edges.value, 1))()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(n_edges)) == 0
    return n_nodes.value, [(src[k], dst[k]) for k in range(n_edges.value)], n_deps.value


def test_score_and_rank_behind_the_chain_in_one_linear_hip_graph():
    cfg = NetConfig(grey=False)
    model = Model(cfg, seed=0)
    lib = _lib.load()
    labels = synthetic.rectangle_maps(3, 4, 32, 32)
    x = torch.from_numpy(synthetic.textured_images(4, labels, 4, 3)).cuda()
    n, cap = 4, 64
    gts = [[[8.0, 8.0, 60.0, 8.0, 60.0, 40.0, 8.0, 40.0], [70.0, 70.0, 120.0, 70.0, 95.0, 120.0]] for _ in range(n)]
    xy, first, _, image_first, max_gt = ev.pack_ground_truth(gts)
    xy_d, first_d = torch.from_numpy(xy).cuda(), torch.from_numpy(first).cuda()
    gt_counts = torch.from_numpy(np.diff(image_first).astype(np.int32)).cuda()
    thr = np.ascontiguousarray(THR, dtype=np.float64)
    need = int(lib.ubd_evaluate_workspace_bytes(n, max_gt, cap, len(thr), 0))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(ev.accumulator_bytes(len(thr), 0), dtype=torch.uint8, device="cuda")
    off, stride = ctypes.c_int64(), ctypes.c_int64()
    assert lib.ubd_evaluate_tables_layout(n, max_gt, cap, len(thr), 0, ctypes.byref(off), ctypes.byref(stride)) == 0
    iou_ptr = ws.data_ptr() + off.value + (max_gt + cap + max_gt * cap) * 8
    logits = torch.empty((n, 32, 32, model.k_out), dtype=torch.float32, device="cuda")
    outs = model.alloc_postprocess_outputs(n, 32, 32, cap)
    scores = torch.empty((n, cap), dtype=torch.float32, device="cuda")
    capacity = 4096
    buf = torch.zeros(ev.rank_buffer_bytes(capacity), dtype=torch.uint8, device="cuda")

    def chain(prepacked):
        model.predict_on_device(x, out=logits, _prepacked=prepacked)
        model.postprocess_on_device(logits, -2.0, 4, 5, cap=cap, outputs=outs)
        assert lib.ubd_evaluate_objects(outs[1].data_ptr(), None, outs[3].data_ptr(), n, cap, None, xy_d.data_ptr(), len(xy), first_d.data_ptr(),
                                        None, image_first.ctypes.data, max_gt, thr.ctypes.data, len(thr), 0, None, acc.data_ptr(),
                                        ws.data_ptr(), need, _stream()) == 0, lib.ubd_last_error()
        model.score_objects_on_device(logits, outs[1], outs[3], 4, out=scores)
        assert lib.ubd_rank_detections(scores.data_ptr(), outs[3].data_ptr(), n, cap, iou_ptr, stride.value, gt_counts.data_ptr(),
                                       thr.ctypes.data, len(thr), buf.data_ptr(), capacity, _stream()) == 0, lib.ubd_last_error()
    chain(False); chain(False)
    torch.cuda.synchronize()
    buf.zero_()
    chain(False)
    torch.cuda.synchronize()
    direct = buf.cpu().numpy().tobytes()
    u = ev.unpack_rank_buffer(np.frombuffer(direct, np.uint8))
    assert u["images"] == n and u["flagged"] == 0 and u["written"] == int(outs[3].sum()) and u["n_gt"] == 2 * n
    buf.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(True)
        n_nodes, edges, open_ends = _capturing_graph_shape()
    # linear: every node of the captured graph has at most one predecessor and one successor, and the capture ends in one node
    sources, targets = [a for a, _ in edges], [b for _, b in edges]
    assert n_nodes >= 6 and len(edges) == n_nodes - 1 and open_ends == 1, (n_nodes, len(edges), open_ends)
    assert len(set(sources)) == len(sources) and len(set(targets)) == len(targets), "the captured graph forks or joins"
    buf.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == direct
    g.replay()                                                      # the buffer keeps filling: the same records twice
    torch.cuda.synchronize()
    twice = ev.unpack_rank_buffer(buf.cpu().numpy())
    assert twice["written"] == 2 * u["written"] and twice["images"] == 2 * n
    assert np.array_equal(twice["tp_mask"], np.concatenate([u["tp_mask"]] * 2))
