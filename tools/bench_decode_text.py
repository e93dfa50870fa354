"""The three patch decoders (ubd_decode_patches, ubd_decode_text_patches, ubd_decode_width_patches) in one run on one MI355X: what
reading Code 128, and ITF and Code 39, as well costs a caller of ModelRunner.predict_decoded(symbologies=7 or 31).

The workload: n = 32 images, cap = 4, every slot filled, one 64 x 256 RGB patch per object at 2 pixels per module with Gaussian
noise (sigma 6, seeded), every other one half-turned: in turn an EAN-13, a Code 128 of five to seven characters, an EAN-8 and a
GS1-128 of eight digits (encoders of tests/decode_cases.py and tests/text_decode_cases.py; the drawn text elements by the rule
of tests/text_decode_oracle.py).  Prints one JSON line per kernel:
HIP-event time per call at the default parameters (5 warm-up calls; windows of --calls back-to-back calls; median, minimum and
90th percentile of --iters windows), patches and counts already in device memory, and how many of the objects of the kernel's
own family decoded to what was drawn (the other family's must all read as none).
The two-width kernel is timed twice: on those patches, which hold nothing of its family (the cost of looking), and on a workload
of its own of the same shape (``width_workload``: in turn an ITF of six to ten digits and a Code 39 of two to four characters,
2 pixels per narrow run, wide runs of 5, the same noise, every other one half-turned).
With --extra, three more pairs of lines follow: UPC-E (bit 6), Code 93 (bit 7) and Codabar (bit 8), each read by its family's
kernel under its own bit alone, once on a workload of its own symbols of the same shape (``extra_workload``: UPC-E and Code 93 of
five to seven characters at 2 pixels per module, Codabar of four to eight data characters at 2 pixels per narrow run and wide
runs of 5) and once on the first workload, where it finds none.  The lines without --extra are unchanged, so that a library from
before these symbologies can be timed beside this one.
Usage: python tools/bench_decode_text.py [--iters 200] [--calls 20] [--extra]
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
import decode_cases as dc  # noqa: E402
import text_decode_cases as tc  # noqa: E402
import text_decode_oracle as to  # noqa: E402
import width_decode_cases as wc  # noqa: E402
import extra_decode_cases as xc  # noqa: E402
from ubdvss_amd import _lib, barcode_decoder  # noqa: E402

ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-/.+"


def workload(n=32, cap=4, ph=64, pw=256, seed=1):
    """-> (patches (n, cap, ph, pw, 3), kinds (n, cap) 'retail' / 'text', drawn (n, cap): the digit list or the value list)"""
    rng = np.random.default_rng(seed)
    patches = np.zeros((n, cap, ph, pw, 3), np.uint8)
    kinds, drawn = np.empty((n, cap), object), np.empty((n, cap), object)
    for i in range(n):
        for j in range(cap):
            which = (i + j) % 4
            if which == 0:
                kinds[i, j], drawn[i, j] = "retail", dc.with_check([int(d) for d in rng.integers(0, 10, 12)])
            elif which == 2:
                kinds[i, j], drawn[i, j] = "retail", dc.with_check([int(d) for d in rng.integers(0, 10, 7)])
            elif which == 1:
                text = "".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), int(rng.integers(5, 8))))
                kinds[i, j], drawn[i, j] = "text", tc.encode_text(text)
            else:
                kinds[i, j], drawn[i, j] = "text", tc.encode_text("".join(str(int(d)) for d in rng.integers(0, 10, 8)), True)
            mods = dc.modules(drawn[i, j]) if kinds[i, j] == "retail" else tc.modules(drawn[i, j])
            row = tc.flat_row_modules([mods], 2, pw, (pw - 2 * len(mods)) // 2).astype(np.float64)
            grey = np.clip(np.rint(row[None, :] + rng.normal(0, 6.0, (ph, pw))), 0, 255).astype(np.uint8)
            if j % 2:
                grey = grey[::-1, ::-1]
            patches[i, j] = grey[:, :, None]
    return patches, kinds, drawn


def width_workload(n=32, cap=4, ph=64, pw=256, seed=2):
    """-> (patches (n, cap, ph, pw, 3), drawn (n, cap): the digits of the ITF or the characters of the Code 39)"""
    rng = np.random.default_rng(seed)
    patches = np.zeros((n, cap, ph, pw, 3), np.uint8)
    drawn = np.empty((n, cap), object)
    for i in range(n):
        for j in range(cap):
            if (i + j) % 2 == 0:
                drawn[i, j] = "".join(str(int(d)) for d in rng.integers(0, 10, 2 * int(rng.integers(3, 6))))
                mods = wc.itf_modules(drawn[i, j], 2, 5)
            else:
                drawn[i, j] = "".join(wc.C39_CHARS[int(k)] for k in rng.integers(0, 43, int(rng.integers(2, 5))))
                mods = wc.c39_modules(drawn[i, j], 2, 5)
            row = tc.flat_row_modules([mods], 1, pw, (pw - len(mods)) // 2).astype(np.float64)
            grey = np.clip(np.rint(row[None, :] + rng.normal(0, 6.0, (ph, pw))), 0, 255).astype(np.uint8)
            if j % 2:
                grey = grey[::-1, ::-1]
            patches[i, j] = grey[:, :, None]
    return patches, drawn


def extra_workload(kind, n=32, cap=4, ph=64, pw=256, seed=3):
    """kind 'upce' / 'code93' / 'codabar' -> (patches (n, cap, ph, pw, 3), drawn (n, cap): the text a record must show)"""
    rng = np.random.default_rng(seed)
    patches = np.zeros((n, cap, ph, pw, 3), np.uint8)
    drawn = np.empty((n, cap), object)
    for i in range(n):
        for j in range(cap):
            if kind == "upce":
                eight = xc.upce_digits(int(rng.integers(0, 2)), [int(d) for d in rng.integers(0, 10, 6)])
                drawn[i, j], mods, px = "".join(map(str, eight)), xc.upce_modules(eight), 2
            elif kind == "code93":
                drawn[i, j] = "".join(xc.C93_ALPHABET[int(k)] for k in rng.integers(0, 43, int(rng.integers(5, 8))))
                mods, px = xc.c93_modules(xc.c93_values(drawn[i, j])), 2
            else:
                data = "".join("0123456789-$:/.+"[int(k)] for k in rng.integers(0, 16, int(rng.integers(4, 9))))
                drawn[i, j] = "ABCD"[int(rng.integers(0, 4))] + data + "ABCD"[int(rng.integers(0, 4))]
                mods, px = xc.cbr_modules(drawn[i, j], 2, 5), 1
            row = tc.flat_row_modules([mods], px, pw, (pw - px * len(mods)) // 2).astype(np.float64)
            grey = np.clip(np.rint(row[None, :] + rng.normal(0, 6.0, (ph, pw))), 0, 255).astype(np.uint8)
            if j % 2:
                grey = grey[::-1, ::-1]
            patches[i, j] = grey[:, :, None]
    return patches, drawn


def time_calls(call, iters, calls):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):                           # one call is tens of microseconds: a window holds several, back to back
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / calls)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--extra", action="store_true", help="also UPC-E, Code 93 and Codabar, each under its own bit")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    n, cap, ph, pw, c = 32, 4, 64, 256, 3
    host_patches, kinds, drawn = workload(n, cap, ph, pw)
    patches = torch.from_numpy(host_patches).cuda()
    counts = torch.full((n,), cap, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    retail = torch.zeros((n, cap, 16), dtype=torch.int32, device="cuda")
    text = torch.zeros((n, cap, 128), dtype=torch.uint8, device="cuda")
    p_retail, p_text = barcode_decoder.make_params(), barcode_decoder.make_params(symbologies=barcode_decoder.CODE128)

    def call_retail():
        _lib.check(lib.ubd_decode_patches(patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(p_retail),
                                          retail.data_ptr(), stream), "ubd_decode_patches")

    def call_text():
        _lib.check(lib.ubd_decode_text_patches(patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(p_text),
                                               text.data_ptr(), stream), "ubd_decode_text_patches")
    width = torch.zeros((n, cap, 128), dtype=torch.uint8, device="cuda")
    p_width = barcode_decoder.make_params(symbologies=barcode_decoder.ITF | barcode_decoder.CODE39)
    host_own, drawn_own = width_workload(n, cap, ph, pw)
    own_patches = torch.from_numpy(host_own).cuda()

    def call_width(which=patches):
        _lib.check(lib.ubd_decode_width_patches(which.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(p_width),
                                                width.data_ptr(), stream), "ubd_decode_width_patches")
    t_retail, t_text = time_calls(call_retail, args.iters, args.calls), time_calls(call_text, args.iters, args.calls)
    t_width = time_calls(call_width, args.iters, args.calls)
    got_width = barcode_decoder.width_results_to_records(width, counts)
    t_own = time_calls(lambda: call_width(own_patches), args.iters, args.calls)
    got_own = barcode_decoder.width_results_to_records(width, counts)
    got_retail = barcode_decoder.results_to_records(retail, counts)
    got_text = barcode_decoder.text_results_to_records(text, counts)
    slots = [(i, j) for i in range(n) for j in range(cap)]
    for name, times, got, kind, right in (
            ("ubd_decode_patches", t_retail, got_retail, "retail", lambda r, d: r.text == "".join(map(str, d))),
            ("ubd_decode_text_patches", t_text, got_text, "text", lambda r, d: r.elements == tuple(to.text_elements(d))),
            ("ubd_decode_width_patches", t_width, got_width, "width", None),
            ("ubd_decode_width_patches_own_workload", t_own, got_own, "own", lambda r, d: r.text == d)):
        own = slots if kind == "own" else [s for s in slots if kinds[s] == kind]
        truth = drawn_own if kind == "own" else drawn
        correct = sum(got[i][j] is not None and right(got[i][j], truth[i, j]) for i, j in own)
        stray = 0 if kind == "own" else sum(got[i][j] is not None for i, j in slots if kinds[i, j] != kind)
        us = float(np.median(times))
        print(json.dumps({"leg": f"{name}_n{n}_cap{cap}_{ph}x{pw}x{c}", "iters": args.iters, "calls_per_window": args.calls,
                          "us_median": round(us, 1), "us_min": round(float(np.min(times)), 1),
                          "us_p90": round(float(np.percentile(times, 90)), 1), "objects": n * cap, "own_family": len(own),
                          "decoded_correctly": int(correct), "other_family_read": int(stray),
                          "objects_per_s": round(n * cap / us * 1e6)}), flush=True)
    if not args.extra:
        return
    for kind, bit, entry, out, to_records in (
            ("upce", barcode_decoder.UPCE, "ubd_decode_patches", retail, barcode_decoder.results_to_records),
            ("code93", barcode_decoder.CODE93, "ubd_decode_text_patches", text, barcode_decoder.text_results_to_records),
            ("codabar", barcode_decoder.CODABAR, "ubd_decode_width_patches", width, barcode_decoder.width_results_to_records)):
        host_kind, drawn_kind = extra_workload(kind, n, cap, ph, pw)
        kind_patches = torch.from_numpy(host_kind).cuda()
        p_kind = barcode_decoder.make_params(symbologies=bit)
        for which, name in ((kind_patches, "own_workload"), (patches, "first_workload")):
            def call(which=which):
                _lib.check(getattr(lib, entry)(which.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(p_kind), out.data_ptr(),
                                               stream), entry)
            times = time_calls(call, args.iters, args.calls)
            got = to_records(out, counts)
            read = sum(got[i][j] is not None for i, j in slots)
            correct = sum(got[i][j] is not None and got[i][j].text == drawn_kind[i, j] for i, j in slots) if name == "own_workload" else 0
            us = float(np.median(times))
            print(json.dumps({"leg": f"{entry}_{kind}_bit{bit}_{name}_n{n}_cap{cap}_{ph}x{pw}x{c}", "iters": args.iters,
                              "calls_per_window": args.calls, "us_median": round(us, 1), "us_min": round(float(np.min(times)), 1),
                              "us_p90": round(float(np.percentile(times, 90)), 1), "objects": n * cap, "read": int(read),
                              "decoded_correctly": int(correct), "objects_per_s": round(n * cap / us * 1e6)}), flush=True)


if __name__ == "__main__":
    main()
