"""Device geometric augmentation (ubd_warp_images) and the augmented training preparation (SegmapManager.prepare_batches_on_device)
on one MI355X.

Prints one JSON line per measurement:
  kernel legs: HIP-event time of one ubd_warp_images call over 64 x 1080 x 1920 frames (median of --iters) for one rotation pass
    and one perspective pass, RGB and grey; bytes moved = source read once + destination written once, and the fraction of
    8 TB/s (the HBM peak) that those bytes are in that time;
  end to end: images/s of prepare_batches_on_device(augment=True) on 64 mixed camera frames (numpy, host) with seeded plans,
    next to (a) the host chain the reference runs -- Pillow rotate + crop + transform + BICUBIC resize + convert('L') +
    ImageDraw label map, on a thread pool, labelled with its core count -- and (b) the plain prepare_batch_on_device on the same
    frames (no augmentation).
The photometric stage is not part of either side of the end-to-end legs (the plans are sampled without a photo_rng).
  --photometric: instead of the legs above, HIP-event time of one ubd_photometric_images call per mode over 16 x 1080 x 1920 RGB
    frames (median of --iters), source and destination in separate buffers, next to the bytes-moved bound of a stage,
    2 x image bytes (read once, written once), and the GB/s those bytes are in that time.
    The legs: every mode, MEDIAN at k = 3 and 11, HSV, ELASTIC at alpha = 3.5 (--only NAME[,NAME]: just those legs).
  --noise-alpha: instead of the legs above, HIP-event time of one ubd_noise_alpha_images call over 32 x 512 x 512 RGB images with
    three 16 x 16 cubic grids, max aggregation and a sigmoid curve, branches FILTER3 / IDENTITY (SimplexNoiseAlpha's shape) and
    AFFINE / AFFINE (FrequencyNoiseAlpha's), next to one ubd_photometric_images call in mode FILTER3 on the same images: the
    three calls alternate inside every round (200 rounds by default), median and minimum per call, and the ratios to FILTER3.
Usage: python tools/bench_augment.py [--iters 30] [--e2e-iters 5] [--photometric [--only median_k11]] [--noise-alpha [--rounds 200]]
"""
import argparse
import concurrent.futures as cf
import ctypes
import json
import os
import random
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ubdvss_amd import _lib, NetConfig, ObjectMarkup, SegmapManager, synthetic  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

HBM_TBS = 8.0


def kernel_leg(name, n, h, w, c, mode, coeffs, dst_size, iters):
    lib = _lib.load()
    src = torch.randint(0, 256, (n * h * w * c,), dtype=torch.uint8, device="cuda")
    dw, dh = dst_size
    per = (dw * dh * c + 255) & ~255
    dst = torch.empty(n * per, dtype=torch.uint8, device="cuda")
    descs = np.zeros(n, aug.WARP_DESC)
    descs["src_offset"] = np.arange(n, dtype=np.int64) * (h * w * c)
    descs["dst_offset"] = np.arange(n, dtype=np.int64) * per
    descs["src_xpitch"], descs["src_ypitch"], descs["src_w"], descs["src_h"] = c, w * c, w, h
    descs["dst_w"], descs["dst_h"], descs["mode"] = dw, dh, mode
    descs["coeffs"][:, :len(coeffs)] = coeffs
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.ubd_warp_images(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), descs.ctypes.data, c, n, stream),
                   "ubd_warp_images")
    for _ in range(3):
        call()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    us = float(np.median(times))
    gb = (n * h * w * c + n * dw * dh * c) / 1e9
    return {"leg": name, "images": n, "src": [h, w, c], "dst": [dh, dw, c], "us_median": round(us, 1), "us_min": round(float(np.min(times)), 1),
            "MB_moved": round(gb * 1e3, 1), "TBps": round(gb / us * 1e3, 3), "fraction_of_8TBps": round(gb / us * 1e3 / HBM_TBS, 3)}


def photometric_legs(iters, n=16, h=1080, w=1920, c=3, only=None):
    lib = _lib.load()
    St = aug.Stage
    stages = [("affine_contrast", St("contrast", {"alphas": (1.7, 0.6, 1.2), "per_channel": True}, None)),
              ("grey", St("grayscale", {"alpha": 0.6}, None)),
              ("filter3_sharpen", St("sharpen", {"alpha": 0.5, "lightness": 1.2}, None)),
              ("sep_gaussian_sigma1_r2", St("gaussian_blur", {"sigma": 1.0}, None)),
              ("sep_gaussian_sigma3_r4", St("gaussian_blur", {"sigma": 3.0}, None)),
              ("box_k2", St("average_blur", {"k": 2}, None)),
              ("box_k7", St("average_blur", {"k": 7}, None)),
              ("noise_shared", St("noise", {"scale": 6.0, "per_channel": False, "seed": 1}, None)),
              ("noise_per_channel", St("noise", {"scale": 6.0, "per_channel": True, "seed": 1}, None)),
              ("dropout_per_channel", St("dropout", {"p": 0.05, "per_channel": True, "seed": 2}, None)),
              ("median_k3", St("median_blur", {"k": 3}, None)),
              ("median_k11", St("median_blur", {"k": 11}, None)),
              ("hsv", St("hue_saturation", {"value": 12}, None)),
              ("elastic_alpha3.5", St("elastic", {"applied": True, "alpha": 3.5, "sigma": 0.25, "seed": 3}, None))]
    if only:
        stages = [(name, st) for name, st in stages if name in only]
    per = h * w * c
    src = torch.randint(0, 256, (n * per,), dtype=torch.uint8, device="cuda")
    dst = torch.empty(n * per, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for name, st in stages:
        f = aug.photometric_descs(st, w, h, c)
        descs = np.zeros(n, aug.PHOTO_DESC)
        descs["src_offset"] = descs["dst_offset"] = np.arange(n, dtype=np.int64) * per
        descs["w"], descs["h"], descs["mode"], descs["flags"], descs["seed"] = w, h, f["mode"], f["flags"], f["seed"]
        descs["p"][:, :len(f["p"])] = f["p"]

        def call():
            _lib.check(lib.ubd_photometric_images(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), descs.ctypes.data, c, n, stream),
                       "ubd_photometric_images")
        for _ in range(3):
            call()
        times = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        us = float(np.median(times))
        gb = 2 * n * per / 1e9
        out.append({"leg": f"photometric_{name}_{n}x{h}p_c{c}", "mode": int(f["mode"]), "us_median": round(us, 1), "us_min": round(float(np.min(times)), 1),
                    "MB_bound_2x_image_bytes": round(gb * 1e3, 1), "GBps": round(gb / us * 1e6, 1),
                    "fraction_of_8TBps": round(gb / us * 1e3 / HBM_TBS, 3)})
    return out


def noise_alpha_legs(rounds, n=32, h=512, w=512, c=3):
    lib = _lib.load()
    St = aug.Stage
    per = h * w * c
    src = torch.randint(0, 256, (n * per,), dtype=torch.uint8, device="cuda")
    dst = torch.empty(n * per, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    its = tuple({"size": 16, "upscale": "cubic", "seed": 10 + k} for k in range(3))
    stages = {"simplex_filter3_identity": St("simplex_alpha", {"directed": True, "alpha": 0.8, "direction": 0.3, "iterations": its, "aggregation": "max",
                                                              "sigmoid": True, "threshold": 1.0}, None),
              "frequency_affine_affine": St("frequency_alpha", {"exponent": -2.0, "factors": (0.7, 1.1, 1.4), "contrast_alpha": 1.6, "iterations": its,
                                                                "aggregation": "max", "sigmoid": True, "threshold": 1.0}, None)}
    calls, keep = {}, []
    for name, st in stages.items():
        f, tab = aug.noise_alpha_descs(st, w, h, c)
        descs = np.zeros(n, aug.NOISE_ALPHA_DESC)
        for k in range(n):
            aug.fill_noise_alpha_desc(descs[k], f)
        descs["src_offset"] = descs["dst_offset"] = np.arange(n, dtype=np.int64) * per
        descs["w"], descs["h"] = w, h
        tables = torch.from_numpy(tab.view(np.int16)).cuda()
        keep.append((descs, tables))
        calls["noise_alpha_" + name] = lambda d=descs, t=tables: _lib.check(
            lib.ubd_noise_alpha_images(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), d.ctypes.data, t.data_ptr(), t.numel(), c, n, stream),
            "ubd_noise_alpha_images")
    f = aug.photometric_descs(St("sharpen", {"alpha": 0.5, "lightness": 1.2}, None), w, h, c)
    pd = np.zeros(n, aug.PHOTO_DESC)
    pd["src_offset"] = pd["dst_offset"] = np.arange(n, dtype=np.int64) * per
    pd["w"], pd["h"], pd["mode"] = w, h, f["mode"]
    pd["p"][:, :len(f["p"])] = f["p"]
    calls["photometric_filter3"] = lambda: _lib.check(
        lib.ubd_photometric_images(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), pd.ctypes.data, c, n, stream), "ubd_photometric_images")
    for fn in calls.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(rounds):                                   # the calls alternate inside every round
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    base = float(np.median(times["photometric_filter3"]))
    gb = 2 * n * per / 1e9
    return [{"leg": f"{name}_{n}x{h}x{w}_c{c}", "rounds": rounds, "us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1),
             "MB_bound_2x_image_bytes": round(gb * 1e3, 1), "GBps": round(gb / float(np.median(t)) * 1e6, 1),
             "ratio_to_photometric_filter3": round(float(np.median(t)) / base, 2)} for name, t in times.items()]


def _pillow_chain(im, plan):
    for st in plan.stages:
        if st.kind in ("rotate", "quarter"):
            im = im.rotate(st.params["angle"], Image.BILINEAR, expand=True)
        elif st.kind == "crop":
            im = im.crop(st.params["box"])
        else:
            im = im.transform(im.size, Image.PERSPECTIVE, st.params["coeffs"], Image.BILINEAR)
    return im


def e2e(iters, threads):
    cfg = NetConfig()                                         # the reference default: grey, 512 max side, multiples of 64
    rng = np.random.default_rng(1)
    sizes = [(1080, 1920), (720, 1280), (1079, 1921), (600, 1100)] * 16
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    markups = [[ObjectMarkup(q.reshape(-1).tolist()) for q in synthetic.random_quads(rng, h, w, 2, 6, 8, 40)] for h, w in sizes]
    plans = [aug.sample_plan((w, h), m, random.Random(k), np.random.RandomState(k)) for k, ((h, w), m) in enumerate(zip(sizes, markups))]
    pool = cf.ThreadPoolExecutor(threads)

    def host_one(k):
        im = _pillow_chain(Image.fromarray(frames[k]), plans[k])
        mk = aug.apply_plan_to_markup(plans[k], markups[k])
        im, mk = SegmapManager._rescale_image_and_markup(im, mk, cfg)
        seg = SegmapManager.build_segmentation_map(im, mk, scale=cfg.get_scale())
        return np.asarray(im.convert("L")), np.asarray(seg)

    def host_chain():
        return list(pool.map(host_one, range(len(frames))))

    def device_augmented():
        return SegmapManager.prepare_batches_on_device(frames, markups, cfg, augment=True, plans=plans)

    def device_plain():
        return SegmapManager.prepare_batch_on_device(frames, markups, cfg)
    res = {}
    for name, fn in (("host_pillow_chain", host_chain), ("prepare_batches_on_device_augmented", device_augmented),
                     ("prepare_batch_on_device_plain", device_plain)):
        fn(); torch.cuda.synchronize()
        t = []
        for _ in range(iters):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
        res[name] = {"ms_median": round(1e3 * float(np.median(t)), 2), "images_per_s": round(len(frames) / float(np.median(t)), 1)}
    host = host_chain()
    same = True
    for idx, x, labels, _, _ in device_augmented():
        xs, ls = x.cpu().numpy(), labels.cpu().numpy()
        same = same and all(np.array_equal(xs[j][..., 0], host[i][0]) and np.array_equal(ls[j], host[i][1]) for j, i in enumerate(idx))
    n_passes = sum(("rotate" in [s.kind for s in p.stages]) + ("perspective" in [s.kind for s in p.stages]) for p in plans)
    return {"leg": "e2e_64_mixed_frames_rgb_to_grey_net_input_and_labels", **res, "host_threads": threads, "host_cores": os.cpu_count(),
            "resampling_passes_in_plans": n_passes,
            "augmented_vs_host": round(res["host_pillow_chain"]["ms_median"] / res["prepare_batches_on_device_augmented"]["ms_median"], 2),
            "augmented_vs_plain": round(res["prepare_batches_on_device_augmented"]["ms_median"] / res["prepare_batch_on_device_plain"]["ms_median"], 2),
            "identical_to_host_chain": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--e2e-iters", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--photometric", action="store_true", help="time ubd_photometric_images per mode instead of the warp / end-to-end legs")
    ap.add_argument("--only", default="", help="with --photometric: comma-separated leg names (e.g. median_k11), for a profiler run of one leg")
    ap.add_argument("--noise-alpha", action="store_true", help="time ubd_noise_alpha_images next to ubd_photometric_images in mode FILTER3")
    ap.add_argument("--rounds", type=int, default=200, help="with --noise-alpha: rounds in which the calls alternate")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.noise_alpha:
        for leg in noise_alpha_legs(args.rounds):
            print(json.dumps(leg), flush=True)
        return
    if args.photometric:
        for leg in photometric_legs(args.iters, only=[v for v in args.only.split(",") if v]):
            print(json.dumps(leg), flush=True)
        return
    _, matrix, size = aug.rotate_matrix_and_size(31.7, (1920, 1080))
    persp = (aug.PERSPECTIVE_MEAN + 0.5 * aug.PERSPECTIVE_HALF).tolist()
    for c in (3, 1):
        print(json.dumps(kernel_leg(f"rotate_31.7deg_64x1080p_c{c}", 64, 1080, 1920, c, _lib.UBD_WARP_AFFINE, matrix, size, args.iters)), flush=True)
        print(json.dumps(kernel_leg(f"perspective_64x1080p_c{c}", 64, 1080, 1920, c, _lib.UBD_WARP_PERSPECTIVE, persp, (1920, 1080), args.iters)),
              flush=True)
    print(json.dumps(e2e(args.e2e_iters, args.host_threads)), flush=True)


if __name__ == "__main__":
    main()
