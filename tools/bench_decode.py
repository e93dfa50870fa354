"""Device decoding of the object patches (ubd_decode_patches) on one MI355X, next to the copy it makes unnecessary.

The workload: n = 32 images, cap = 16, 4 objects each, one 64 x 256 RGB patch per object holding a noisy EAN-13 or EAN-8 at
2 pixels per module (seeded), every other one half-turned.  Prints one JSON line per leg:
  kernel: HIP-event time per ubd_decode_patches call at the default parameters (5 warm-up calls; windows of --calls
    back-to-back calls, median and minimum of --iters windows), patches and counts already in device memory; the bytes of the
    objects' patches read per second; how many of the objects decoded to the digits drawn;
  copies: the device -> pinned host copy of the objects' patches (n, 4, 64, 256, 3), which ModelRunner.predict_patches makes and
    predict_decoded does not, and of the (n, 4, 16) int32 results that predict_decoded reads instead; host clock around copy
    and synchronise, median of --copy-iters.
Usage: python tools/bench_decode.py [--iters 200] [--calls 20] [--copy-iters 50]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ubdvss_amd import _lib, barcode_decoder  # noqa: E402

L_CODES = ["0001101", "0011001", "0010011", "0111101", "0100011", "0110001", "0101111", "0111011", "0110111", "0001011"]
PARITY = ["LLLLLL", "LLGLGG", "LLGGLG", "LLGGGL", "LGLLGG", "LGGLLG", "LGGGLL", "LGLGLG", "LGLGGL", "LGGLGL"]


def symbol_modules(body):
    """12 or 7 digits -> (all digits, the modules as a list of 0 / 1)"""
    total = sum(d * (3 if k % 2 == 0 else 1) for k, d in enumerate(reversed(body)))
    digits = list(body) + [(10 - total % 10) % 10]
    r_code = ["".join("1" if ch == "0" else "0" for ch in s) for s in L_CODES]
    g_code = [s[::-1] for s in r_code]
    if len(digits) == 13:
        left = "".join((L_CODES if p == "L" else g_code)[d] for p, d in zip(PARITY[digits[0]], digits[1:7]))
        right = "".join(r_code[d] for d in digits[7:])
    else:
        left, right = "".join(L_CODES[d] for d in digits[:4]), "".join(r_code[d] for d in digits[4:])
    return digits, [int(ch) for ch in "101" + left + "01010" + right + "101"]


def workload(n=32, cap=16, per=4, ph=64, pw=256, seed=1):
    rng = np.random.default_rng(seed)
    patches = np.zeros((n, cap, ph, pw, 3), np.uint8)
    want = np.full((n, per, 13), -1, np.int64)
    for i in range(n):
        for j in range(per):
            digits, mods = symbol_modules([int(d) for d in rng.integers(0, 10, 12 if (i + j) % 3 else 7)])
            want[i, j, :len(digits)] = digits
            row = np.full(pw, 225.0)
            start = (pw - 2 * len(mods)) // 2
            for k, m in enumerate(mods):
                if m:
                    row[start + 2 * k:start + 2 * k + 2] = 35.0
            grey = np.clip(np.rint(row[None, :] + rng.normal(0, 6.0, (ph, pw))), 0, 255).astype(np.uint8)
            if j % 2:
                grey = grey[::-1, ::-1]
            patches[i, j] = grey[:, :, None]
    return patches, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--copy-iters", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    n, cap, per, ph, pw, c = 32, 16, 4, 64, 256, 3
    host_patches, want = workload(n, cap, per, ph, pw)
    patches = torch.from_numpy(host_patches).cuda()
    counts = torch.full((n,), per, dtype=torch.int32, device="cuda")
    results = torch.zeros((n, cap, 16), dtype=torch.int32, device="cuda")
    params = barcode_decoder.make_params()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.ubd_decode_patches(patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params),
                                          results.data_ptr(), stream), "ubd_decode_patches")
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
    got = results.cpu().numpy()[:, :per]
    correct = int(sum(np.array_equal(got[i, j, 3:], want[i, j]) for i in range(n) for j in range(per)))
    read_bytes = n * per * ph * pw * c
    print(json.dumps({"leg": f"ubd_decode_patches_n{n}_cap{cap}_{per}_objects_each_{ph}x{pw}x{c}", "iters": args.iters,
                      "calls_per_window": args.calls, "us_median": round(us, 1), "us_min": round(float(np.min(times)), 1),
                      "us_p90": round(float(np.percentile(times, 90)), 1), "objects": n * per, "decoded_correctly": correct,
                      "MB_read": round(read_bytes / 1e6, 2), "GBps_read": round(read_bytes / us / 1e3, 1),
                      "objects_per_s": round(n * per / us * 1e6)}), flush=True)

    def copy_ms(src):
        dst = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        out = []
        for k in range(args.copy_iters + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            if k >= 3:
                out.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(out)), float(np.min(out))
    objects = patches[:, :per].contiguous()
    p_med, p_min = copy_ms(objects)
    r_med, r_min = copy_ms(results[:, :per].contiguous())
    print(json.dumps({"leg": "device_to_pinned_host_copies", "iters": args.copy_iters, "patches_MB": round(objects.numel() / 1e6, 2),
                      "patches_copy_us_median": round(p_med * 1e3, 1), "patches_copy_us_min": round(p_min * 1e3, 1),
                      "results_bytes": n * per * 64, "results_copy_us_median": round(r_med * 1e3, 1),
                      "results_copy_us_min": round(r_min * 1e3, 1),
                      "kernel_plus_results_copy_over_patches_copy": round((us + r_med * 1e3) / (p_med * 1e3), 3)}), flush=True)


if __name__ == "__main__":
    main()
