"""Device extraction of rectified object patches (ubd_extract_objects) on one MI355X, next to the host alternative.

The workload: 32 frames of 1080 x 1920 RGB, 8 objects each (rotated rectangles of about 300 x 100 pixels at seeded positions and
angles), one 64 x 256 patch per object.  Prints one JSON line per leg:
  kernel: HIP-event time per ubd_extract_objects call (5 warm-up calls; windows of --calls back-to-back calls, median and minimum
    of --iters windows), frames, quads, counts and descriptors already in device memory; output bytes written per second;
  host: what a decoder's feeder does without the kernel -- the frames copied device -> host (one copy, timed with a
    synchronise) plus one Image.transform((256, 64), QUAD, data, BILINEAR) per object on one core (median of --host-iters);
  and whether the two produce the same bytes.
Usage: python tools/bench_extract.py [--iters 200] [--calls 20] [--host-iters 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import _lib  # noqa: E402


def workload(n=32, per=8, h=1080, w=1920, seed=1):
    rng = np.random.default_rng(seed)
    quads = np.zeros((n, per, 8), np.int32)
    for i in range(n):
        for j in range(per):
            t = rng.uniform(0, np.pi)
            cx, cy = rng.uniform(200, w - 200), rng.uniform(200, h - 200)
            ux, uy = np.array([np.cos(t), np.sin(t)]) * 150, np.array([-np.sin(t), np.cos(t)]) * 50
            pts = [np.array([cx, cy]) + a * ux + b * uy for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            quads[i, j] = np.rint(np.array(pts)).astype(np.int32).reshape(-1)
    return quads


def oriented(q):
    """the corner order of ubd_extract_objects (include/ubd.h) for one quad: clockwise, a long side first"""
    p = [(int(q[2 * k]), int(q[2 * k + 1])) for k in range(4)]
    if sum(p[k][0] * p[(k + 1) % 4][1] - p[(k + 1) % 4][0] * p[k][1] for k in range(4)) < 0:
        p = [p[0], p[3], p[2], p[1]]
    e01 = (p[1][0] - p[0][0]) ** 2 + (p[1][1] - p[0][1]) ** 2
    e12 = (p[2][0] - p[1][0]) ** 2 + (p[2][1] - p[1][1]) ** 2
    r = 0 if e01 >= e12 else 1
    return [p[(r + k) % 4] for k in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--host-iters", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    n, per, h, w, c, ph, pw = 32, 8, 1080, 1920, 3, 64, 256
    quads = workload(n, per, h, w)
    frames = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * (h * w * c)
    hw = torch.tensor([[h, w]] * n, dtype=torch.int32, device="cuda")
    quads_d = torch.from_numpy(quads).cuda()
    counts = torch.full((n,), per, dtype=torch.int32, device="cuda")
    patches = torch.zeros((n, per, ph, pw, c), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.ubd_extract_objects(frames.data_ptr(), frames.numel(), offs.data_ptr(), hw.data_ptr(), c, quads_d.data_ptr(),
                                           counts.data_ptr(), n, per, None, 1.0, patches.data_ptr(), ph, pw, None, stream),
                   "ubd_extract_objects")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):                      # one call is tens of microseconds: a window holds several, back to back
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / args.calls)
    us = float(np.median(times))
    out_bytes = n * per * ph * pw * c
    print(json.dumps({"leg": f"ubd_extract_objects_{n}x{h}p_c{c}_{per}_objects_each_{ph}x{pw}", "iters": args.iters, "calls_per_window": args.calls, "us_median": round(us, 1),
                      "us_min": round(float(np.min(times)), 1), "us_p90": round(float(np.percentile(times, 90)), 1),
                      "patches": n * per, "MB_written": round(out_bytes / 1e6, 2), "GBps_written": round(out_bytes / us / 1e3, 1),
                      "patches_per_s": round(n * per / us * 1e6)}), flush=True)
    got = patches.cpu().numpy()

    def host():
        t0 = time.perf_counter()
        fh = frames.cpu().numpy()                        # .cpu() synchronises
        t1 = time.perf_counter()
        res = np.empty((n, per, ph, pw, c), np.uint8)
        for i in range(n):
            im = Image.fromarray(fh[i])
            for j in range(per):
                nw, ne, se, sw = oriented(quads[i, j])
                res[i, j] = np.asarray(im.transform((pw, ph), Image.QUAD, nw + sw + se + ne, Image.BILINEAR))
        return t1 - t0, time.perf_counter() - t1, res
    host()
    runs = [host() for _ in range(args.host_iters)]
    copy_ms, pil_ms = 1e3 * float(np.median([r[0] for r in runs])), 1e3 * float(np.median([r[1] for r in runs]))
    print(json.dumps({"leg": "host_copy_back_plus_pillow_quad_bilinear_one_core", "iters": args.host_iters, "copy_back_ms_median": round(copy_ms, 2),
                      "pillow_ms_median": round(pil_ms, 2), "total_ms_median": round(copy_ms + pil_ms, 2),
                      "ratio_to_kernel": round((copy_ms + pil_ms) * 1e3 / us, 1), "identical_to_kernel": bool(np.array_equal(runs[-1][2], got))}),
          flush=True)


if __name__ == "__main__":
    main()
