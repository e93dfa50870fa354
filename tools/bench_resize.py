"""Device bicubic resize (ubd_resize_images) and raw-image inference (ModelRunner.predict_images) on one MI355X.

Prints one JSON line per measurement:
  kernel legs: HIP-event time of one ubd_resize_images call (median of --iters), source bytes read and the fraction of the
    6.29 TB/s measured copy rate that those bytes are in that time;
  end to end: frames/s of predict_images on 32 raw 1080p RGB frames (numpy, host) against the host chain the reference runs
    -- Pillow BICUBIC resize + convert('L') on a 16-thread pool, then ModelRunner.predict on the uint8 batch.
Usage: python tools/bench_resize.py [--iters 50] [--e2e-iters 10]
"""
import argparse
import concurrent.futures as cf
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import _lib, NetConfig, Model, ModelRunner, SegmapManager  # noqa: E402

COPY_TBS = 6.29


def kernel_leg(name, sizes, src_c, dst_h, dst_w, dst_c, iters):
    lib = _lib.load()
    rng = np.random.default_rng(0)
    nbytes = [h * w * src_c for h, w in sizes]
    offs = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    src = torch.from_numpy(rng.integers(0, 256, int(sum(nbytes)), dtype=np.uint8)).cuda()
    hw = np.array(sizes, np.int32)
    dst = torch.empty((len(sizes), dst_h, dst_w, dst_c), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.ubd_resize_images(src.data_ptr(), offs.ctypes.data, hw.ctypes.data, src_c, len(sizes), dst.data_ptr(),
                                         dst_h, dst_w, dst_c, stream), "ubd_resize_images")
    for _ in range(5):
        call()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    us = float(np.median(times))
    gb = sum(nbytes) / 1e9
    return {"leg": name, "images": len(sizes), "src_c": src_c, "dst": [dst_h, dst_w, dst_c], "us_median": round(us, 1),
            "us_min": round(float(np.min(times)), 1), "src_MB": round(gb * 1e3, 1),
            "src_TBps": round(gb / us * 1e3, 3), "fraction_of_copy_rate": round(gb / us * 1e3 / COPY_TBS, 3)}


def e2e(iters):
    cfg = NetConfig()                                         # the reference default: grey, 512 max side, multiples of 64
    model = Model(cfg, seed=0)
    runner = ModelRunner(cfg)
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(32)]
    pool = cf.ThreadPoolExecutor(16)

    def host_prep(a):
        im = Image.fromarray(a)
        w, h = im.size
        r, _ = SegmapManager._rescale_image_and_markup(im, None, cfg)
        return np.asarray(r.convert("L"))[..., None], (w / r.size[0], h / r.size[1])

    class Meta:
        def __init__(self, s): self.xscale, self.yscale = s

    def host_chain():
        out = list(pool.map(host_prep, frames))
        x = np.stack([o[0] for o in out])
        return runner.predict(model, x, rescale=True, meta_infos=[Meta(o[1]) for o in out])[2]

    def device_chain():
        return runner.predict_images(model, frames)
    res = {}
    for name, fn in (("host_chain", host_chain), ("predict_images", device_chain)):
        fn(); torch.cuda.synchronize()
        t = []
        for _ in range(iters):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
        res[name] = {"ms_median": round(1e3 * float(np.median(t)), 2), "frames_per_s": round(32 / float(np.median(t)), 1)}
    same = [[tuple(o.bbox) for o in f] for f in host_chain()] == [[tuple(o.bbox) for o in f] for f in device_chain()]
    return {"leg": "e2e_32x1080p_raw_rgb_to_objects", **res, "speedup": round(res["host_chain"]["ms_median"] / res["predict_images"]["ms_median"], 2),
            "objects_identical": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--e2e-iters", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    legs = [("32x1080p_rgb_to_512x256_L", [(1080, 1920)] * 32, 3, 256, 512, 1),
            ("32x1080p_rgb_to_512x256_rgb", [(1080, 1920)] * 32, 3, 256, 512, 3),
            ("32x480p_rgb_to_512x384_L", [(480, 640)] * 32, 3, 384, 512, 1),
            ("32_mixed_rgb_to_512x256_L", [(1080, 1920), (720, 1280), (1079, 1921), (600, 1100)] * 8, 3, 256, 512, 1)]
    for leg in legs:
        print(json.dumps(kernel_leg(*leg, iters=args.iters)), flush=True)
    print(json.dumps(e2e(args.e2e_iters)), flush=True)


if __name__ == "__main__":
    main()
