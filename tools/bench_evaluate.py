"""Device object-level evaluation (ubd_evaluate_objects) on one MI355X.

Prints one JSON line per measurement (HIP-event time, median of --iters calls after a warm-up):
  (a) ubd_evaluate_objects alone: 32 and 64 images with 1-8 objects each and with 64 objects each, twelve thresholds;
  (b) forward + postprocess + evaluation against forward + postprocess of the same batch of 32 images of 512 x 512, in the
      same run: what the evaluation adds to the step that precedes it;
      -- once with the bare C-ABI call on buffers made beforehand (ground truth packed and uploaded, workspace allocated: the
      device cost), once through the public DatasetMetricCalculator.evaluate_batch, which validates, packs and uploads the
      ground truth and allocates the workspace on every batch (event time and wall clock with a synchronisation, since that
      part is host work);
  (c) for orientation only, the host alternative: copy the object lists back and score them with a plain fp64 Python / NumPy
      version of the same rule (score_image_fp64 below; wall clock, one core).
  (d) ubd_evaluate_pixels: 32 maps of 128 x 128 and 8 maps of 256 x 256 with three classes (the LDS form and the global-memory
      form), the bare C-ABI call on buffers made beforehand and the public evaluate_pixels wrapper (which allocates the
      workspace and the outputs per call); beside it, in the same run, stand-alone ubd_postprocess on logits whose detection
      channel draws the SAME maps (the same labelling plus a box fit), and the host alternative: copy logits and labels back
      and run the numpy / oracle.cv_post restatement on one core (wall clock).
Usage: python tools/bench_evaluate.py [--iters 20] [--only-pixels]
       rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_evaluate.py --trace-loop 50
         (only the 32-image, 1-8-object call, 50 times: the per-kernel split of profiles/r09_evaluate_kernel_stats.csv)
       rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_evaluate.py --trace-loop-pixels 50
         (both pixel cases, 50 times each: profiles/r10_evaluate_pixels_kernel_stats.csv)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import _lib, NetConfig, Model, ModelRunner, ObjectMarkup, synthetic  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

THRESHOLDS = ev.DatasetMetricCalculator.IOU_THRESHOLDS


# ---- the same rule on the host in fp64 ---------------------------------------------------------------------------------------------
def _ccw(p):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    r = p - p[0]
    a = 0.5 * float(np.sum(r[:, 0] * np.roll(r[:, 1], -1) - r[:, 1] * np.roll(r[:, 0], -1)))
    if a < 0:
        p = np.concatenate([p[:1], p[:0:-1]])
        a = -a
    return p, a


def _interval(ax, ay, bx, by, P, same_inside):
    lo, hi = 0.0, 1.0
    px, py = P[-1]
    for qx, qy in P:
        ex, ey = qx - px, qy - py
        d0 = ex * (ay - py) - ey * (ax - px)
        d1 = ex * (by - py) - ey * (bx - px)
        px, py = qx, qy
        if ex == 0.0 and ey == 0.0:
            continue
        if d0 == 0.0 and d1 == 0.0:
            if same_inside and ex * (bx - ax) + ey * (by - ay) > 0.0:
                continue
            return None
        if d0 <= 0.0 and d1 <= 0.0:
            return None
        if d0 < 0.0:
            lo = max(lo, d0 / (d0 - d1))
        elif d1 < 0.0:
            hi = min(hi, d0 / (d0 - d1))
    return (lo, hi) if lo < hi else None


def _inter(Pg, ag, Pf, af):
    if not (ag > 0 and af > 0):
        return 0.0
    rx, ry = Pg[0]
    tot = 0.0
    for A, B, same in ((Pg, Pf, True), (Pf, Pg, False)):
        for k in range(len(A)):
            (ax, ay), (bx, by) = A[k], A[(k + 1) % len(A)]
            iv = _interval(ax, ay, bx, by, B, same)
            if iv:
                tot += (iv[1] - iv[0]) * (0.5 * ((ax - rx) * (by - ry) - (ay - ry) * (bx - rx)))
    return min(max(tot, 0.0), min(ag, af))


def _union(polys):
    """polys: list of (index, vertices, area); the boundary integral with covered parts removed"""
    polys = [p for p in polys]
    if not polys:
        return 0.0
    rx, ry = polys[0][1][0]
    tot = 0.0
    for si, Pi, ai in polys:
        if not ai > 0:
            continue
        for k in range(len(Pi)):
            (ax, ay), (bx, by) = Pi[k], Pi[(k + 1) % len(Pi)]
            if ax == bx and ay == by:
                continue
            ivs = []
            for sj, Pj, aj in polys:
                if sj != si and aj > 0:
                    iv = _interval(ax, ay, bx, by, Pj, sj < si)
                    if iv:
                        ivs.append(iv)
            ivs.sort()
            free, pos = 0.0, 0.0
            for lo, hi in ivs:
                if lo > pos:
                    free += lo - pos
                pos = max(pos, hi)
            free += max(0.0, 1.0 - pos)
            tot += free * (0.5 * ((ax - rx) * (by - ry) - (ay - ry) * (bx - rx)))
    return max(tot, 0.0)


def _iou(a1, a2, it):
    u = a1 + a2 - it
    return it / u if u > 0 else 0.0


def score_image_fp64(gts, founds, thresholds, gt_cls=None, found_cls=None, n_classes=0):
    """One image: list per threshold of dicts with the record fields (+ 'confusion' with classes)."""
    g = [_ccw(p) for p in gts]
    f = [_ccw(p) for p in founds]
    G, F = len(g), len(f)
    inter = np.zeros((G, F))
    iou = np.zeros((G, F))
    for i in range(G):
        for j in range(F):
            inter[i, j] = _inter(g[i][0], g[i][1], f[j][0], f[j][1])
            iou[i, j] = _iou(g[i][1], f[j][1], inter[i, j])
    adj = iou > 0.05
    ngf, nfg = adj.sum(1), adj.sum(0)
    gp = [(i, g[i][0], g[i][1]) for i in range(G)]
    fp_ = [(G + j, f[j][0], f[j][1]) for j in range(F)]

    def group_iou(group, box):
        a_grp, a_all = _union(group), _union(sorted(group + [box]))
        it = min(max(a_grp + box[2] - a_all, 0.0), min(a_grp, box[2]))
        return _iou(a_grp, box[2], it)
    o2o, o2m, m2o = [], [], []
    for i in range(G):
        idx = np.nonzero(adj[i])[0]
        if len(idx) == 1 and nfg[idx[0]] == 1:
            o2o.append((i, idx[0], iou[i, idx[0]]))
        elif len(idx) > 1 and all(nfg[j] == 1 for j in idx):
            o2m.append((i, idx, group_iou([fp_[j] for j in idx], gp[i])))
    for j in range(F):
        idx = np.nonzero(adj[:, j])[0]
        if len(idx) > 1 and all(ngf[i] == 1 for i in idx):
            m2o.append((idx, j, group_iou([gp[i] for i in idx], fp_[j])))
    aG, aF, aA = _union(gp), _union(fp_), _union(gp + fp_)
    it = min(max(aG + aF - aA, 0.0), min(aG, aF))
    p_area, r_area, iou_area = (it / aF if aF > 0 else 0.0), (it / aG if aG > 0 else 0.0), _iou(aG, aF, it)
    C = n_classes if gt_cls is not None and found_cls is not None else 0
    out = []
    for thr in thresholds:
        cm = np.zeros((C, C))
        mg = mf = boxes = n11 = n1m = nm1 = 0
        s = 0.0
        for i, j, v in o2o:
            if v >= thr:
                n11 += 1; s += v
                if C:
                    cm[gt_cls[i], found_cls[j]] += 1
        mg = mf = boxes = n11
        for i, idx, v in o2m:
            if v >= thr:
                mg += 1; n1m += 1; mf += len(idx); boxes += 1; s += v
                if C:
                    tot = 0.0
                    for j in idx:
                        tot += inter[i, j]
                    for j in idx:
                        cm[gt_cls[i], found_cls[j]] += inter[i, j] / tot
        for idx, j, v in m2o:
            if v >= thr:
                mg += len(idx); nm1 += len(idx); mf += 1; boxes += 1; s += v
                if C:
                    for i in idx:
                        cm[gt_cls[i], found_cls[j]] += 1
        out.append(dict(tp=mg, fp=F - mf, fn=G - mg, one_to_one=n11, one_to_many=n1m, many_to_one=nm1, matched_boxes_count=boxes,
                        detection_rate=int(iou_area > thr), iou_sum=s, precision_by_area=p_area, recall_by_area=r_area,
                        iou_by_area=iou_area, confusion=cm))
    return out


# ---- measurements --------------------------------------------------------------------------------------------------------------------
def _objects(rng, n, lo, hi, side=2048):
    """per image lo..hi ground-truth quads and as many found quads (jittered copies): (gts, quads (n, cap, 8), counts)"""
    cap = max(hi, 1)
    quads = np.zeros((n, cap, 8), dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    gts = []
    for i in range(n):
        k = int(rng.integers(lo, hi + 1))
        q = np.array(synthetic.random_quads(rng, side, side, k, k, 2, 10)).reshape(k, 8)
        gts.append([row.astype(np.float64).tolist() for row in q])
        quads[i, :k] = np.round(q + rng.uniform(-4, 4, q.shape)).astype(np.int32)
        counts[i] = k
    return gts, quads, counts


def _time(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(times)), 1), round(float(np.min(times)), 1)


def _wall(call, iters):
    """median wall-clock microseconds of call + synchronisation: what a host-bound path costs the loop that runs it"""
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter(); call(); torch.cuda.synchronize(); times.append(1e6 * (time.perf_counter() - t0))
    return round(float(np.median(times)), 1)


class _RawCall:
    """ubd_evaluate_objects with every buffer made once: what is timed is the call, not the packing of the ground truth"""

    def __init__(self, quads_d, classes_d, counts_d, gts, n_classes=0):
        self.lib = _lib.load()
        dev = quads_d.device
        self.n, self.cap = int(quads_d.shape[0]), int(quads_d.shape[1])
        xy, first, _, self.image_first, self.max_gt = ev.pack_ground_truth(gts)
        self.n_vertices = len(xy)
        self.xy, self.first = torch.from_numpy(xy).to(dev), torch.from_numpy(first).to(dev)
        self.thr = np.ascontiguousarray(THRESHOLDS, dtype=np.float64)
        self.C = n_classes
        self.quads, self.classes, self.counts = quads_d, classes_d, counts_d
        self.acc = torch.zeros(ev.accumulator_bytes(len(self.thr), self.C), dtype=torch.uint8, device=dev)
        self.need = int(self.lib.ubd_evaluate_workspace_bytes(self.n, self.max_gt, self.cap, len(self.thr), self.C))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev)

    def __call__(self):
        _lib.check(self.lib.ubd_evaluate_objects(
            self.quads.data_ptr(), None, self.counts.data_ptr(), self.n, self.cap, None, self.xy.data_ptr(), self.n_vertices,
            self.first.data_ptr(), None, self.image_first.ctypes.data, self.max_gt, self.thr.ctypes.data, len(self.thr), self.C, None,
            self.acc.data_ptr(), self.ws.data_ptr(), self.need, torch.cuda.current_stream().cuda_stream), "ubd_evaluate_objects")


def leg_alone(n, lo, hi, iters):
    rng = np.random.default_rng(n * 100 + hi)
    gts, quads, counts = _objects(rng, n, lo, hi)
    call = _RawCall(torch.from_numpy(quads).cuda(), None, torch.from_numpy(counts).cuda(), gts)
    med, mn = _time(call, iters)
    t0 = time.perf_counter()
    qh, ch = call.quads.cpu().numpy(), call.counts.cpu().numpy()
    for i in range(n):
        score_image_fp64(gts[i], [qh[i, j] for j in range(ch[i])], THRESHOLDS)
    host_ms = 1e3 * (time.perf_counter() - t0)
    return {"leg": f"evaluate_alone_{n}_images_{lo}_to_{hi}_objects", "objects": int(counts.sum()), "thresholds": len(THRESHOLDS),
            "us_median": med, "us_min": mn, "host_copy_and_fp64_python_ms": round(host_ms, 1)}


def leg_pipeline(iters, n=32, side=512):
    cfg = NetConfig(grey=False)
    model = Model(cfg, seed=0)
    runner = ModelRunner(cfg)
    labels = synthetic.rectangle_maps(7, n, side // 4, side // 4)
    x = torch.from_numpy(synthetic.textured_images(11, labels, 4, 3)).cuda()
    rng = np.random.default_rng(3)
    gts, _, _ = _objects(rng, n, 1, 8, side)
    out = {}

    def fwd_pp():
        out["r"] = runner.predict_on_device(model, x)
    fwd_pp()
    _, _, quads, _, counts = out["r"]
    call = _RawCall(quads, None, counts, gts)

    def fwd_pp_eval():
        _, _, q, _, c = runner.predict_on_device(model, x)
        call.quads, call.counts = q, c
        call()
    calc = ev.DatasetMetricCalculator(cfg)
    gt_objects = [[ObjectMarkup(p) for p in g] for g in gts]

    def fwd_pp_eval_public():
        _, _, q, _, c = runner.predict_on_device(model, x)
        calc.evaluate_batch(gt_objects, (q, None, c))
    a_med, a_min = _time(fwd_pp, iters)
    b_med, b_min = _time(fwd_pp_eval, iters)
    e_med, e_min = _time(call, iters)
    p_med, p_min = _time(fwd_pp_eval_public, iters)
    wall = [_wall(f, iters) for f in (fwd_pp, fwd_pp_eval, fwd_pp_eval_public)]
    return {"leg": f"forward_postprocess_evaluate_{n}x{side}x{side}", "found_objects": int(counts.clamp(max=quads.shape[1]).sum().item()),
            "ground_truth_objects": sum(len(g) for g in gts),
            "forward_postprocess_us_median": a_med, "forward_postprocess_evaluate_us_median": b_med, "evaluate_alone_us_median": e_med,
            "added_us": round(b_med - a_med, 1), "us_min": [a_min, b_min, e_min],
            "public_evaluate_batch": {"forward_postprocess_evaluate_us_median": p_med, "us_min": p_min, "added_us": round(p_med - a_med, 1)},
            "wall_us_median_with_sync": {"forward_postprocess": wall[0], "plus_c_abi_call": wall[1], "plus_public_evaluate_batch": wall[2]}}


class _RawPixelCall:
    """ubd_evaluate_pixels with every buffer made once"""

    def __init__(self, logits_d, labels_d, n_classes):
        self.lib = _lib.load()
        self.z, self.labels, self.C = logits_d, labels_d, n_classes
        self.n, self.h, self.w = (int(v) for v in labels_d.shape)
        self.need = int(self.lib.ubd_evaluate_pixels_workspace_bytes(self.n, self.h, self.w))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=logits_d.device)
        self.acc = torch.zeros(ev.pixel_accumulator_bytes(), dtype=torch.uint8, device=logits_d.device)
        self.mask = torch.empty((self.n, self.h, self.w), dtype=torch.int8, device=logits_d.device)

    def __call__(self):
        _lib.check(self.lib.ubd_evaluate_pixels(self.z.data_ptr() + 4, self.C + 1, self.C, self.labels.data_ptr(), self.n, self.h, self.w,
                                                self.mask.data_ptr(), None, self.acc.data_ptr(), self.ws.data_ptr(), self.need,
                                                torch.cuda.current_stream().cuda_stream), "ubd_evaluate_pixels")


def _pixel_inputs(n, side, n_classes=3):
    """label maps of textured-rectangle scenes and net-shaped logits: the detection channel draws the same maps (for the
    postprocess beside it), the class channels favour the true class"""
    labels = synthetic.rectangle_maps(17 + side, n, side, side, n_classes=n_classes).astype(np.int32).reshape(n, side, side)
    rng = np.random.default_rng(side)
    z = rng.normal(size=(n, side, side, 1 + n_classes)).astype(np.float32)
    z[..., 0] = np.where(labels > 0, 5.0, -5.0)
    np.put_along_axis(z, np.where(labels > 0, labels, 1)[..., None], 1.0, axis=-1)
    return labels, z


def _host_pixels(z, labels):
    """the host alternative: evaluation.py:546-575 with numpy and the sequential contour routines of oracle/cv_post.c"""
    from oracle import cv_post as ocv
    mask = labels > 0
    correct = np.where(mask, labels - 1, 0) == np.argmax(z[..., 1:], axis=-1)
    accs = []
    for i in range(len(labels)):
        h, w = mask[i].shape
        for cnt in ocv.find_contours(mask[i].astype(np.uint8), approx_simple=False):
            accs.append(correct[i][ocv.fill_contour(cnt, h, w).astype(bool)].mean())
    return int((correct & mask).sum()), int(mask.sum()), len(accs), float(np.sum(accs))


def leg_pixels(n, side, iters, model):
    labels, z = _pixel_inputs(n, side)
    zd, ld = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda()
    call = _RawPixelCall(zd, ld, 3)
    med, mn = _time(call, iters)
    acc = torch.zeros(ev.pixel_accumulator_bytes(), dtype=torch.uint8, device="cuda")
    pub_med, pub_min = _time(lambda: ev.evaluate_pixels(zd, ld, acc, want_mask=True, n_classes=3, per_image=False), iters)
    pub_wall = _wall(lambda: ev.evaluate_pixels(zd, ld, acc, want_mask=True, n_classes=3, per_image=False), iters)
    outs = model.alloc_postprocess_outputs(n, side, side, 256)
    pp_med, pp_min = _time(lambda: model.postprocess_on_device(zd, 0.0, 4, 5, cap=256, outputs=outs), iters)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = _host_pixels(zd.cpu().numpy(), ld.cpu().numpy())
    host_ms = 1e3 * (time.perf_counter() - t0)
    call.acc.zero_(); call(); torch.cuda.synchronize()
    a = ev.unpack_pixel_accumulator(call.acc.cpu().numpy())
    assert (a["n_correct"], a["n_total"], a["n_objects"]) == host[:3], (a, host)
    return {"leg": f"evaluate_pixels_{n}_maps_{side}x{side}_3_classes", "form": "lds" if side * side <= 16384 else "global",
            "objects": a["n_objects"], "logit_bytes": int(z.nbytes), "us_median": med, "us_min": mn,
            "public_evaluate_pixels": {"us_median": pub_med, "us_min": pub_min, "wall_us_median_with_sync": pub_wall},
            "standalone_postprocess_same_maps": {"us_median": pp_med, "us_min": pp_min, "found": int(outs[3].clamp(max=256).sum().item())},
            "host_copy_and_numpy_oracle_ms": round(host_ms, 1)}


PIXEL_CASES = ((32, 128), (8, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-pixels", action="store_true", help="only the ubd_evaluate_pixels legs")
    ap.add_argument("--trace-loop-pixels", type=int, default=0, help="only N calls of each pixel case (for a kernel trace)")
    ap.add_argument("--trace-loop", type=int, default=0, help="only N calls of the 32-image 1-8-object case (for a kernel trace)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.trace_loop:
        gts, quads, counts = _objects(np.random.default_rng(3208), 32, 1, 8)
        call = _RawCall(torch.from_numpy(quads).cuda(), None, torch.from_numpy(counts).cuda(), gts)
        for _ in range(args.trace_loop):
            call()
        torch.cuda.synchronize()
        return
    if args.trace_loop_pixels:
        for n, side in PIXEL_CASES:
            labels, z = _pixel_inputs(n, side)
            call = _RawPixelCall(torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda(), 3)
            for _ in range(args.trace_loop_pixels):
                call()
            torch.cuda.synchronize()
        return
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    if not args.only_pixels:
        for n in (32, 64):
            for lo, hi in ((1, 8), (64, 64)):
                print(json.dumps(leg_alone(n, lo, hi, args.iters)), flush=True)
        print(json.dumps(leg_pipeline(args.iters)), flush=True)
    pp_model = Model(NetConfig(class_names=["a", "b", "c"], grey=False), seed=0)
    for n, side in PIXEL_CASES:
        print(json.dumps(leg_pixels(n, side, args.iters, pp_model)), flush=True)


if __name__ == "__main__":
    main()
