"""Times the polygon ground-truth calls on the GPU.  Needs an MI355X; there is no CPU path.

  segmap    ubd_segmap_polygons on 64 maps of 640 x 480 with 4..8 rotated rectangles each
  evaluate  on the same found lists (64 images): ubd_evaluate_objects with quad ground truth, ubd_evaluate_polygons(max_verts = 64)
            with the same quads (bit-identical results, only the slot stride differs) and with hull ground truth of 9..64 vertices

Each figure: device events around ``--calls`` back-to-back calls after ``--warmup`` calls, buffers made once; the median of
``--repeats`` such windows and their spread.  ``--quad-only --root DIR`` times only ubd_evaluate_objects with the package found
in DIR: the way to put another build's quad path beside these numbers in one session.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np


def rotated_rects(rng, h, w, count):
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    quads = []
    for k in range(count):
        cx, cy = (k % 4 + 0.5) * w / 4 + rng.uniform(-20, 20), (k // 4 + 0.5) * h / 2 + rng.uniform(-30, 30)
        a, b, ang = rng.uniform(30, 60), rng.uniform(15, 40), rng.uniform(0, np.pi)
        u = (xs - cx) * np.cos(ang) + (ys - cy) * np.sin(ang)
        v = -(xs - cx) * np.sin(ang) + (ys - cy) * np.cos(ang)
        m[(np.abs(u) <= a) & (np.abs(v) <= b)] = 255
        c, s = np.cos(ang), np.sin(ang)
        quads.append([int(round(cx + dx * c - dy * s)) if i == 0 else int(round(cy + dx * s + dy * c))
                      for dx, dy in ((-a, -b), (a, -b), (a, b), (-a, b)) for i in (0, 1)])
    return m, quads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--quad-only", action="store_true")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    from ubdvss_amd import _lib
    from ubdvss_amd import evaluation as ev
    if not torch.cuda.is_available():
        raise SystemExit("bench_polygons needs an MI355X")
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0 / args.calls)
        return dict(us_median=round(float(np.median(out)), 2), us_min=round(min(out), 2), us_max=round(max(out), 2))

    n, h, w = 64, 480, 640
    rng = np.random.default_rng(1)
    made = [rotated_rects(rng, h, w, int(rng.integers(4, 9))) for _ in range(n)]
    maps = np.stack([m for m, _ in made])
    result = dict(images=n, map=[h, w], calls=args.calls, repeats=args.repeats)
    gt_quads = [q for _, q in made]
    found = [[[v + int(d) for v, d in zip(q, rng.integers(-6, 7, 8))] for q in qs] for qs in gt_quads]
    fq, _, fc = ev.pack_found_objects([[q for q in f if ev._is_convex(np.asarray(q, float).reshape(4, 2))] for f in found])
    fq_d, fc_d = torch.from_numpy(fq).cuda(), torch.from_numpy(fc).cuda()
    thr = np.ascontiguousarray(ev.DatasetMetricCalculator.IOU_THRESHOLDS, dtype=np.float64)
    T, cap = len(thr), int(fq.shape[1])

    def evaluator(gts, polygons):
        xy = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for g in gts for p in g]))
        first = np.cumsum([0] + [len(p) // 2 for g in gts for p in g]).astype(np.int32)
        image_first = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
        max_gt = max(len(g) for g in gts)
        xy_d, first_d = torch.from_numpy(xy).cuda(), torch.from_numpy(first).cuda()
        acc = torch.zeros(ev.accumulator_bytes(T, 0), dtype=torch.uint8, device="cuda")
        need = int(lib.ubd_evaluate_polygons_workspace_bytes(n, max_gt, cap, T, 0, 64) if polygons
                   else lib.ubd_evaluate_workspace_bytes(n, max_gt, cap, T, 0))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        head = (fq_d.data_ptr(), None, fc_d.data_ptr(), n, cap, None, xy_d.data_ptr(), len(xy), first_d.data_ptr(), None,
                image_first.ctypes.data, max_gt, thr.ctypes.data, T, 0)
        tail = (None, acc.data_ptr(), ws.data_ptr(), need, stream)
        keep = (xy_d, first_d, acc, ws, image_first)

        def call():
            rc = lib.ubd_evaluate_polygons(*head, 64, *tail) if polygons else lib.ubd_evaluate_objects(*head, *tail)
            assert rc == 0, (lib.ubd_last_error(), keep is None)
        return call, acc

    call_q, acc_q = evaluator(gt_quads, False)
    result["evaluate_objects_quads"] = timed(call_q)
    if not args.quad_only:
        maps_d = torch.from_numpy(maps).cuda()
        cap_p = 64
        need = int(lib.ubd_segmap_polygons_workspace_bytes(n, h, w, cap_p))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        verts = torch.zeros((n, cap_p, 64, 2), dtype=torch.int32, device="cuda")
        nverts = torch.zeros((n, cap_p), dtype=torch.int32, device="cuda")
        counts = torch.zeros((n,), dtype=torch.int32, device="cuda")

        def segmap():
            assert lib.ubd_segmap_polygons(maps_d.data_ptr(), n, h, w, verts.data_ptr(), nverts.data_ptr(), counts.data_ptr(), cap_p,
                                           ws.data_ptr(), need, stream) == 0, lib.ubd_last_error()
        result["segmap_polygons"] = timed(segmap)
        vh, nh, ch = verts.cpu().numpy(), nverts.cpu().numpy(), counts.cpu().numpy()
        hulls = [[vh[i, o, :nh[i, o]].reshape(-1).tolist() for o in range(ch[i]) if 3 <= nh[i, o] <= 64] for i in range(n)]
        result["hull_vertices"] = dict(max=int(nh.max()), median=float(np.median(nh[nh > 0])), objects=int(ch.sum()))
        call_p, acc_p = evaluator(gt_quads, True)
        result["evaluate_polygons_quads"] = timed(call_p)
        acc_q.zero_(); acc_p.zero_()
        call_q(); call_p()
        torch.cuda.synchronize()
        result["quads_bit_identical"] = bool(acc_q.cpu().numpy().tobytes() == acc_p.cpu().numpy().tobytes())
        call_h, _ = evaluator(hulls, True)
        result["evaluate_polygons_hulls"] = timed(call_h)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
