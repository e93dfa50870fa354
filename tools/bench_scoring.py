"""Detection scores and ranked records (ubd_score_objects, ubd_rank_detections) on one MI355X, beside ubd_evaluate_objects.

Prints one JSON line per capacity (HIP-event time, median of --iters calls after a warm-up): a batch of 32 maps of 128 x 128
(images of 512 x 512 at scale 4) whose images hold as many ground-truth and found objects as the committed evaluation cases
(tests/eval_cases.py, batch(SEED_INT, 1)): random rotated boxes as found objects, jittered copies as ground truth, logits that
draw the boxes.  Every buffer is made once: what is timed is the C-ABI call.  The evaluate call is timed on the same batch; the
rank call reads the IoU tables that call left in its workspace.
Usage: python tools/bench_scoring.py [--iters 50]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_cases as ec  # noqa: E402
from ubdvss_amd import _lib, synthetic  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402
from bench_evaluate import _RawCall, _time  # noqa: E402

THRESHOLDS = ev.DatasetMetricCalculator.IOU_THRESHOLDS
N, MAP, SCALE = 32, 128, 4


def _batch(cap):
    """(logits (N, MAP, MAP, 1), quads (N, cap, 8), counts (N), gts) with the object counts of the committed cases"""
    cases = ec.batch(ec.SEED_INT, 1)
    rng = np.random.default_rng(77)
    side = MAP * SCALE
    quads = np.zeros((N, cap, 8), np.int32)
    counts = np.zeros(N, np.int32)
    gts = []
    maps = np.zeros((N, MAP, MAP), np.int32)
    for i in range(N):
        g_case, f_case = cases[i % len(cases)]
        k = min(len(f_case), cap)
        q = np.array(synthetic.random_quads(rng, side, side, max(k, 1), max(k, 1), 6, 50)).reshape(-1, 8)     # sides of 24..200 image pixels
        quads[i, :k] = np.round(q[:k]).astype(np.int32)
        counts[i] = k
        im = Image.new(mode="L", size=(MAP, MAP), color=0)
        for row in quads[i, :k]:
            ImageDraw.Draw(im).polygon([(int(x) // SCALE, int(y) // SCALE) for x, y in row.reshape(4, 2)], fill=1)
        maps[i] = np.asarray(im, dtype=np.int32)
        g = []
        for j in range(len(g_case)):                                # a found box shrunk and shifted as a whole: convex like the box
            box = q[j % len(q)].reshape(4, 2)
            ctr = box.mean(axis=0)
            g.append(((box - ctr) * rng.uniform(0.7, 1.0) + ctr + rng.uniform(-6, 6, 2)).reshape(-1).tolist())
        gts.append(g)
    logits = synthetic.logits_from_maps(maps, 0, seed=5, noise=1.0)
    return logits, quads, counts, gts


def leg(cap, iters):
    lib = _lib.load()
    logits, quads, counts, gts = _batch(cap)
    lt, qt, ct = torch.from_numpy(logits).cuda(), torch.from_numpy(quads).cuda(), torch.from_numpy(counts).cuda()
    scores = torch.empty((N, cap), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def score():
        _lib.check(lib.ubd_score_objects(lt.data_ptr(), 1, qt.data_ptr(), ct.data_ptr(), N, MAP, MAP, cap, SCALE, scores.data_ptr(), stream),
                   "ubd_score_objects")
    evaluate = _RawCall(qt, None, ct, gts)
    off, stride = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.ubd_evaluate_tables_layout(N, evaluate.max_gt, cap, len(THRESHOLDS), 0, ctypes.byref(off), ctypes.byref(stride)),
               "ubd_evaluate_tables_layout")
    iou_ptr = evaluate.ws.data_ptr() + off.value + (evaluate.max_gt + cap + evaluate.max_gt * cap) * 8
    gt_counts = torch.from_numpy(np.array([len(g) for g in gts], np.int32)).cuda()
    thr = np.ascontiguousarray(THRESHOLDS, dtype=np.float64)
    capacity = 1 << 20
    buf = torch.zeros(ev.rank_buffer_bytes(capacity), dtype=torch.uint8, device="cuda")

    def rank():
        _lib.check(lib.ubd_rank_detections(scores.data_ptr(), ct.data_ptr(), N, cap, iou_ptr, stride.value, gt_counts.data_ptr(),
                                           thr.ctypes.data, len(thr), buf.data_ptr(), capacity, stream), "ubd_rank_detections")
    score(); evaluate()
    e_med, e_min = _time(evaluate, iters)
    s_med, s_min = _time(score, iters)
    r_med, r_min = _time(rank, iters)
    torch.cuda.synchronize()
    u = ev.unpack_rank_buffer(buf.cpu().numpy())
    assert u["dropped"] == 0 and u["flagged"] == 0
    return {"leg": f"score_rank_evaluate_{N}_maps_{MAP}x{MAP}_cap_{cap}", "found_objects": int(counts.sum()),
            "ground_truth_objects": sum(len(g) for g in gts), "thresholds": len(thr),
            "score_objects_us_median": s_med, "rank_detections_us_median": r_med, "evaluate_objects_us_median": e_med,
            "us_min": [s_min, r_min, e_min], "mean_score": round(float(scores.sum().item()) / max(int(counts.sum()), 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    for cap in (64, 256):
        print(json.dumps(leg(cap, args.iters)), flush=True)


if __name__ == "__main__":
    main()
