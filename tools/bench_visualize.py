"""Device visualisations (ubd_visualize_images) on one MI355X.

Times the four-output call at N = 32, 512 x 512 x 3 uint8 images, 128 x 128 maps and 1-8 found quads per image (the textured
rectangle scenes of ubdvss_amd/synthetic.py; the quads are the boxes ubd_postprocess finds on the label maps).  Prints one JSON
line per measurement (HIP-event time, median of --iters calls after a warm-up):
  (a) the bare C-ABI call on buffers made beforehand, with
        compulsory bytes = N H W (C + 4 * 3) + the three maps + the quads, and the fraction of the byte bound they make at
        8 TB/s (the HBM peak of MI355X_MICROARCH; the whole working set of 130 MB also fits the 256 MiB Infinity Cache, so
        the figure is a share of the HBM bound, not proof of HBM traffic);
  (b) the public Visualizer.compute_visualizations_on_device (allocates the four outputs per call), event time and wall clock;
  (c) the host alternative on the same machine: the device-to-host copy of the inputs plus the Pillow calls of
      tests/visualization_oracle.py on one core (wall clock) -- what a user does without this call.
Usage: python tools/bench_visualize.py [--iters 20] [--n 32] [--side 512]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ubdvss_amd import _lib, SegmapManager, Visualizer, synthetic  # noqa: E402
import visualization_oracle as vo  # noqa: E402

HBM_BYTES_PER_S = 8e12


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
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter(); call(); torch.cuda.synchronize(); times.append(1e6 * (time.perf_counter() - t0))
    return round(float(np.median(times)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--side", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_visualize needs an MI355X: a time taken elsewhere says nothing")
    torch.cuda.set_device(0)
    n, side, scale, cap = args.n, args.side, 4, 256
    m = side // scale
    labels = synthetic.rectangle_maps(7, n, m, m, n_classes=3).astype(np.int32)
    images = synthetic.textured_images(11, labels, scale, 3)
    rng = np.random.default_rng(3)
    cls = np.where(labels > 0, np.where(rng.random(labels.shape) < 0.8, 1, -1), 0).astype(np.int8)
    quads = np.zeros((n, cap, 8), np.int32)
    counts = np.zeros(n, np.int32)
    for i in range(n):                                              # the boxes the postprocess finds on these maps
        objs = SegmapManager.postprocess((labels[i] > 0).astype(np.int32)[..., None], None, scale=scale, min_area_threshold=5)
        counts[i] = len(objs)
        for j, o in enumerate(objs[:cap]):
            quads[i, j] = np.asarray(o.bbox, dtype=np.int32)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (images, labels, (labels > 0).astype(np.int32), quads, counts, cls)]
    x, gt, seg, q, c, mask = d
    outs = [torch.empty((n, side, side, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
    lib = _lib.load()

    def raw():
        _lib.check(lib.ubd_visualize_images(x.data_ptr(), _lib.UBD_IN_U8, _lib.UBD_PRE_NONE, n, side, side, 3, m, m, gt.data_ptr(), seg.data_ptr(),
                                            q.data_ptr(), c.data_ptr(), cap, mask.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                            outs[2].data_ptr(), outs[3].data_ptr(), torch.cuda.current_stream().cuda_stream), "ubd_visualize_images")

    def public():
        return Visualizer.compute_visualizations_on_device(x, gt, seg, (q, c), mask)

    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    med, mn = _time(raw, args.iters)
    live_quads = int(np.minimum(counts, cap).sum())
    compulsory = n * side * side * (3 + 4 * 3) + n * m * m * (4 + 4 + 1) + live_quads * 32 + n * 4
    bound_us = compulsory / HBM_BYTES_PER_S * 1e6
    print(json.dumps({"leg": f"visualize_four_outputs_{n}x{side}x{side}x3_maps_{m}x{m}", "quads": live_quads, "us_median": med, "us_min": mn,
                      "compulsory_bytes": compulsory, "byte_bound_us_at_8TBps": round(bound_us, 1),
                      "fraction_of_byte_bound": round(bound_us / med, 3), "achieved_TBps": round(compulsory / med / 1e6, 2)}), flush=True)
    p_med, p_min = _time(public, args.iters)
    print(json.dumps({"leg": "public_compute_visualizations_on_device", "us_median": p_med, "us_min": p_min,
                      "wall_us_median_with_sync": _wall(public, args.iters)}), flush=True)
    # the device call and the Pillow calls draw the same pixels (checked on the first two images)
    raw(); torch.cuda.synchronize()
    want = vo.pillow_all(images[:2], labels[:2], (labels[:2] > 0), quads[:2], counts[:2], cls[:2])
    for k, o in zip(("gt", "seg_map", "postprocessed", "classification_gt"), outs):
        assert np.array_equal(o[:2].cpu().numpy(), want[k]), k
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [t.cpu().numpy() for t in (x, gt, seg, q, c, mask)]
    t1 = time.perf_counter()
    vo.pillow_all(host[0], host[1], host[2], host[3], host[4], host[5])
    t2 = time.perf_counter()
    print(json.dumps({"leg": "host_alternative_copy_inputs_and_pillow_one_core", "copy_ms": round(1e3 * (t1 - t0), 1),
                      "pillow_ms": round(1e3 * (t2 - t1), 1), "total_ms": round(1e3 * (t2 - t0), 1),
                      "times_the_device_call": round(1e6 * (t2 - t0) / med, 0)}), flush=True)


if __name__ == "__main__":
    main()
