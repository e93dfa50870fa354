"""The postal patch decoder (ubd_decode_postal_patches) beside the three older ones on one MI355X, and two builds of the library
in turn inside one process: what reading POSTNET, PLANET, RM4SCC and KIX as well costs a caller of
ModelRunner.predict_decoded(symbologies=479 | 15360), and whether the older kernels moved.

Two workloads of n = 32 images, cap = 4, every slot filled, one 64 x 256 RGB patch per object, every other one half-turned:
the first workload of tools/bench_decode_text.py (retail and Code 128 symbols: nothing postal in it), and ``postal_workload``:
in turn a POSTNET of five or nine digits, a PLANET of eleven, an RM4SCC of six to eight characters and a KIX of eight to twelve,
drawn by tests/postal_decode_cases.py at pitch 4 with 2-pixel bars and Gaussian noise (sigma 6, seeded).
Per library (--lib name=path, any number; default: the package's own) and leg one JSON line: HIP-event time per call (5 warm-up
calls; windows of --calls back-to-back calls; median, minimum and 90th percentile over --rounds x --iters windows, the libraries
taking turns round by round), patches and counts already in device memory.  The legs: the three older entries on the first
workload at masks 3, 4 and 24; the postal entry (mask 15360, scan_rows 16) on the first workload, where it finds nothing, and
on its own, with the number of objects read as drawn; ubd_decode_width_patches at mask 24 on the postal workload, beside it.
A library without the postal entry (a build of the parent commit) runs the older legs only.
Usage: python tools/bench_decode_postal.py [--lib new=ubdvss_amd/libubd_hip.so --lib parent=tools/_ab/parent.so] [--rounds 5] [--iters 40] [--calls 20]
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
import postal_decode_cases as pc  # noqa: E402
from bench_decode_text import time_calls, workload  # noqa: E402
from ubdvss_amd import _lib, barcode_decoder as bd  # noqa: E402

ENTRIES = ("ubd_decode_patches", "ubd_decode_text_patches", "ubd_decode_width_patches", "ubd_decode_postal_patches")


def postal_workload(n=32, cap=4, ph=64, pw=256, seed=4):
    """-> (patches (n, cap, ph, pw, 3), drawn (n, cap): the text a record must show)"""
    rng = np.random.default_rng(seed)
    patches = np.zeros((n, cap, ph, pw, 3), np.uint8)
    drawn = np.empty((n, cap), object)
    letters = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    for i in range(n):
        for j in range(cap):
            which = (i + j) % 4
            if which == 0:
                digits = "".join(str(int(d)) for d in rng.integers(0, 10, 5 if rng.integers(0, 2) else 9))
                drawn[i, j], bars = digits + str(pc.postnet_check(digits)), pc.postnet_bars(digits)
            elif which == 1:
                digits = "".join(str(int(d)) for d in rng.integers(0, 10, 11))
                drawn[i, j], bars = digits + str(pc.postnet_check(digits)), pc.planet_bars(digits)
            elif which == 2:
                text = "".join(letters[int(k)] for k in rng.integers(0, 36, int(rng.integers(6, 9))))
                drawn[i, j], bars = text + pc.rm4scc_check(text), pc.rm4scc_bars(text)
            else:
                text = "".join(letters[int(k)] for k in rng.integers(0, 36, int(rng.integers(8, 13))))
                drawn[i, j], bars = (bd.kix_half_turned(text) if j % 2 else text), pc.kix_bars(text)     # a KIX is read as it lies
            patches[i, j] = pc.render(bars, 4.0, 2.0, h=ph, w=pw, noise=6.0, seed=int(rng.integers(0, 1 << 30)), turned=bool(j % 2), channels=3)
    return patches, drawn


def load(path):
    """a build of the library by path, without the package's symbol table: the parent's build lacks the postal entry"""
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
    n, cap, ph, pw, c = 32, 4, 64, 256, 3
    first = torch.from_numpy(workload(n, cap, ph, pw)[0]).cuda()
    host_postal, drawn = postal_workload(n, cap, ph, pw)
    postal = torch.from_numpy(host_postal).cuda()
    counts = torch.full((n,), cap, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros((n, cap, 128), dtype=torch.uint8, device="cuda")    # 8192 bytes a slot image: room for the retail rows of 64 bytes too
    legs = [("ubd_decode_patches", "mask3_first_workload", first, bd.make_params(symbologies=3)),
            ("ubd_decode_text_patches", "mask4_first_workload", first, bd.make_params(symbologies=4)),
            ("ubd_decode_width_patches", "mask24_first_workload", first, bd.make_params(symbologies=24)),
            ("ubd_decode_width_patches", "mask24_postal_workload", postal, bd.make_params(symbologies=24)),
            ("ubd_decode_postal_patches", "mask15360_first_workload", first, bd.make_params(symbologies=15360, scan_rows=16)),
            ("ubd_decode_postal_patches", "mask15360_postal_workload", postal, bd.make_params(symbologies=15360, scan_rows=16))]
    times, read = {}, {}
    for _ in range(args.rounds):
        for name, (lib, have) in libs:
            for entry, leg, patches, params in legs:
                if entry not in have:
                    continue

                def call():
                    if getattr(lib, entry)(patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(params), out.data_ptr(), stream):
                        raise RuntimeError(lib.ubd_last_error().decode())
                times.setdefault((name, entry, leg), []).extend(time_calls(call, args.iters, args.calls))
                if entry == "ubd_decode_postal_patches":
                    got = bd.postal_results_to_records(out, counts)
                    flat = [(got[i][j], drawn[i, j]) for i in range(n) for j in range(cap)]
                    own = patches is postal
                    read[(name, entry, leg)] = (sum(r is not None for r, _ in flat), sum(own and r is not None and r.text == d for r, d in flat))
    for (name, entry, leg), t in times.items():
        us = float(np.median(t))
        line = {"lib": name, "leg": f"{entry}_{leg}_n{n}_cap{cap}_{ph}x{pw}x{c}", "windows": len(t), "calls_per_window": args.calls,
                "us_median": round(us, 1), "us_min": round(float(np.min(t)), 1), "us_p90": round(float(np.percentile(t, 90)), 1),
                "objects": n * cap, "objects_per_s": round(n * cap / us * 1e6)}
        if (name, entry, leg) in read:
            line["read"], line["read_as_drawn"] = read[(name, entry, leg)]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
