"""The Data Matrix patch decoder (ubd_decode_matrix_patches) beside the four older ones on one MI355X, and two builds of the
library in turn inside one process: what reading Data Matrix as well costs a caller of
ModelRunner.predict_decoded(symbologies=... | 32768, patch_size=(128, 128)), and whether the older kernels moved.

``matrix_workload``: 128 patches (n = 32 images, cap = 4, every slot filled) of 128 x 128 x 3, the nine sizes in turn with random
digit-and-letter texts, at 4 pixels a module (3 for every other symbol up to 22 x 22), the four quarter turns in turn, at -2..2
degrees, degraded as the acceptance set of tests/test_matrix_decode_host.py is (blur 0.7, ramp 25 %, noise sigma 5, seeded).
The older entries run on the workloads of tools/bench_decode_postal.py (64 x 256 x 3), as they did there.
Per library (--lib name=path, any number; default: the package's own) and leg one JSON line: HIP-event time per call (5 warm-up
calls; windows of --calls back-to-back calls; median, minimum and 90th percentile over --rounds x --iters windows, the libraries
taking turns round by round), patches and counts already in device memory; the matrix legs with the number of objects read
as drawn.  A library without the matrix entry (a build of the parent commit) runs the older legs only.
Usage: python tools/bench_decode_matrix.py [--lib new=ubdvss_amd/libubd_hip.so --lib parent=tools/_ab/parent.so] [--rounds 5] [--iters 40] [--calls 20]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import matrix_decode_cases as mc  # noqa: E402
from bench_decode_postal import postal_workload  # noqa: E402
from bench_decode_text import time_calls, workload  # noqa: E402
from ubdvss_amd import _lib, barcode_decoder as bd  # noqa: E402

ENTRIES = ("ubd_decode_patches", "ubd_decode_text_patches", "ubd_decode_width_patches", "ubd_decode_postal_patches", "ubd_decode_matrix_patches")
LETTERS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ -./"


def matrix_workload(n=32, cap=4, side=128, seed=7):
    """-> (patches (n, cap, side, side, 3), drawn (n, cap): (text, size, turns) a record must show)"""
    rng = np.random.default_rng(seed)
    patches = np.zeros((n, cap, side, side, 3), np.uint8)
    drawn = np.empty((n, cap), object)
    for i in range(n):
        for j in range(cap):
            k = i * cap + j
            size = mc.SIZES[k % 9]
            text = ""
            while len(mc.codewords(text)) < mc.CAPACITY[size][0] - (k % 3):      # a new character adds one codeword at the most
                text += LETTERS[int(rng.integers(0, len(LETTERS)))]
            ppm = 3 if size <= 22 and (k // 9) % 2 else 4
            turns = k % 4
            patches[i, j] = mc.render(mc.symbol(text, size), ppm, h=side, w=side, angle=int(rng.integers(-2, 3)), turns=turns,
                                      seed=int(rng.integers(0, 1 << 30)), channels=3, **mc.DEGRADED)
            drawn[i, j] = (text, size, turns)
    return patches, drawn


def load(path):
    """a build of the library by path, without the package's symbol table: the parent's build lacks the matrix entry"""
    lib = ctypes.CDLL(path)
    lib.ubd_last_error.restype = ctypes.c_char_p
    have = []
    for name in ENTRIES:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES["ubd_decode_patches"]
            have.append(name)
    return lib, have


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="name=path of a build of the library; repeat for several")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    libs = [(spec.split("=", 1)[0], load(os.path.abspath(spec.split("=", 1)[1]))) for spec in args.lib] or [("package", load(_lib.LIB_PATH))]
    n, cap, c = 32, 4, 3
    first = torch.from_numpy(workload(n, cap, 64, 256)[0]).cuda()
    postal = torch.from_numpy(postal_workload(n, cap, 64, 256)[0]).cuda()
    host_matrix, drawn = matrix_workload(n, cap, 128)
    matrix = torch.from_numpy(host_matrix).cuda()
    junk = torch.from_numpy(np.random.default_rng(3).integers(0, 256, host_matrix.shape, dtype=np.uint8)).cuda()
    counts = torch.full((n,), cap, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros((n, cap, 128), dtype=torch.uint8, device="cuda")    # room for the retail rows of 64 bytes too
    legs = [("ubd_decode_patches", "mask3_first_workload", first, bd.make_params(symbologies=3)),
            ("ubd_decode_text_patches", "mask4_first_workload", first, bd.make_params(symbologies=4)),
            ("ubd_decode_width_patches", "mask24_first_workload", first, bd.make_params(symbologies=24)),
            ("ubd_decode_postal_patches", "mask15360_postal_workload", postal, bd.make_params(symbologies=15360, scan_rows=16)),
            ("ubd_decode_matrix_patches", "mask32768_noise", junk, bd.make_params(symbologies=32768)),
            ("ubd_decode_matrix_patches", "mask32768_matrix_workload", matrix, bd.make_params(symbologies=32768))]
    times, read = {}, {}
    for _ in range(args.rounds):
        for name, (lib, have) in libs:
            for entry, leg, patches, params in legs:
                if entry not in have:
                    continue
                ph, pw = int(patches.shape[2]), int(patches.shape[3])

                def call():
                    if getattr(lib, entry)(patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params), out.data_ptr(), stream):
                        raise RuntimeError(lib.ubd_last_error().decode())
                times.setdefault((name, entry, leg, ph, pw), []).extend(time_calls(call, args.iters, args.calls))
                if entry == "ubd_decode_matrix_patches":
                    got = bd.matrix_results_to_records(out, counts)
                    flat = [(got[i][j], drawn[i, j]) for i in range(n) for j in range(cap)]
                    own = patches is matrix
                    read[(name, entry, leg, ph, pw)] = (sum(r is not None for r, _ in flat),
                                                        sum(own and r is not None and (r.text, r.size, r.turns) == d for r, d in flat))
    for (name, entry, leg, ph, pw), t in times.items():
        us = float(np.median(t))
        line = {"lib": name, "leg": f"{entry}_{leg}_n{n}_cap{cap}_{ph}x{pw}x{c}", "windows": len(t), "calls_per_window": args.calls,
                "us_median": round(us, 1), "us_min": round(float(np.min(t)), 1), "us_p90": round(float(np.percentile(t, 90)), 1),
                "objects": n * cap, "objects_per_s": round(n * cap / us * 1e6)}
        if (name, entry, leg, ph, pw) in read:
            line["read"], line["read_as_drawn"] = read[(name, entry, leg, ph, pw)]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
