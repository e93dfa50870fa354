"""GPU: ubd_noise_alpha_images (csrc/noise_alpha.hip) -- two processed copies of an image blended by an upscaled noise mask --
and its place in the device augmentation chain against the numpy oracle that defines it (tests/noise_alpha_oracle.py),
np.array_equal throughout, no tolerance: L / RGB images from 1 x 1 up to two 64 x 16 tiles on both axes, grids from 1 x 1 to
16 x 16 (larger than the image among them) with random and 0 / 32768-only values, every upscale method, 1..3 grids with mixed
methods, both aggregations, identity / sigmoid / random monotone curves, every pair of branch kinds, sources at +0 / +1 / +3 and
destinations at +0 / +2 from a dword boundary with guard bytes; known answers that need no oracle of their own; one call over
several launches, graph capture, every limit refused.  Then the chain: augment_arrays_on_device with plans sampled with
photo_extended=True and photo_noise_alpha=True equals Pillow's geometric chain followed by the oracles' stages."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import photometric_oracle as po  # noqa: E402
import photometric_ext_oracle as pe  # noqa: E402
import noise_alpha_oracle as no  # noqa: E402
from ubdvss_amd import NetConfig, ObjectMarkup, SegmapManager, _lib, synthetic  # noqa: E402
from ubdvss_amd import augmentation as aug  # noqa: E402

pytestmark = pytest.mark.gpu

# (w, h); the kernel's tile is 64 x 16: the edge, one over, two tiles on both axes
SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (11, 11), (63, 17), (64, 16), (65, 17), (130, 33)]
GRIDS = [(1, 1), (1, 16), (16, 1), (2, 2), (3, 7), (16, 16)]            # (gh, gw)
IDENT_CURVE = 64 * np.arange(257)
KINDS = (no.IDENTITY, no.FILTER3, no.AFFINE)


def _branch(kind, rng):
    if kind == no.FILTER3:
        which = int(rng.integers(0, 3))
        if which == 0:                                                   # EdgeDetect at a drawn alpha
            a = float(rng.uniform(0.5, 1.0))
            return kind, [int(np.rint(v * 16384)) for v in (0, a, 0, a, 1 - 5 * a, a, 0, a, 0)]
        if which == 1:                                                   # the limits
            return kind, [int(v) for v in rng.choice([-13 * 16384, 13 * 16384, 0, 1], 9)]
        return kind, [int(v) for v in rng.integers(-20000, 20001, 9)]
    if kind == no.AFFINE:
        if rng.random() < 0.3:                                           # the limits
            return kind, [int(v) for v in rng.choice([-(1 << 17), 1 << 17], 3)] + [int(v) for v in rng.choice([-(1 << 24), 1 << 24, 0], 3)]
        return kind, [int(v) for v in rng.integers(20000, 120000, 3)] + [int(v) for v in rng.integers(-(1 << 22), 1 << 22, 3)]
    return kind, []


def _grid(rng, shape, extreme=False):
    return (rng.integers(0, 2, shape) * 32768 if extreme else rng.integers(0, 32769, shape)).astype(np.uint16)


def _curve(which, rng):
    if which == 0:
        return IDENT_CURVE
    if which == 1:
        return aug.alpha_curve(True, float(rng.uniform(-6, 6))).astype(np.int64)       # steep: most of the range is 0 or 16384
    return np.sort(rng.integers(0, 16385, 257))


def _spec(rng, grids, pair, aggregation, curve):
    return {"first": _branch(pair[0], rng), "second": _branch(pair[1], rng), "grids": grids, "aggregation": aggregation,
            "curve": np.asarray(curve, np.int64)}


def _want(img, s):
    return no.apply(img, s["first"], s["second"], s["grids"], s["aggregation"], s["curve"])


def _tables_and_descs(jobs, offs, doffs):
    """the uint16 table array of all jobs and their descriptors"""
    tabs, pos = [], 0
    descs = np.zeros(len(jobs), aug.NOISE_ALPHA_DESC)
    for k, (a, s) in enumerate(jobs):
        d = descs[k]
        d["src_offset"], d["dst_offset"], d["w"], d["h"] = offs[k], doffs[k], a.shape[1], a.shape[0]
        d["iterations"], d["aggregation"] = len(s["grids"]), s["aggregation"]
        for name in ("first", "second"):
            d[name]["kind"] = s[name][0]
            d[name]["p"][:len(s[name][1])] = s[name][1]
        for i, (g, up) in enumerate(s["grids"]):
            d["grid"][i]["gh"], d["grid"][i]["gw"], d["grid"][i]["upscale"], d["grid"][i]["grid_offset"] = g.shape[0], g.shape[1], up, pos
            tabs.append(np.asarray(g, np.uint16).reshape(-1))
            pos += g.size
        d["curve_offset"] = pos
        tabs.append(np.asarray(s["curve"], np.uint16))
        pos += 257
    return np.concatenate(tabs), descs


def _call(lib, src_ptr, src_bytes, dst_ptr, dst_bytes, descs, tables, c, stream=None):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    _lib.check(lib.ubd_noise_alpha_images(src_ptr, src_bytes, dst_ptr, dst_bytes, descs.ctypes.data, tables.data_ptr(), tables.numel(),
                                          c, len(descs), st), "ubd_noise_alpha_images")


def _device(jobs, c, misalign=(0, 1, 3), dst_misalign=(0, 2)):
    """jobs: [(image, spec)].  All sources in one device buffer at +0 / +1 / +3 from a dword boundary, destinations at +0 / +2
    with guard bytes between them, checked; the sources must come back unwritten (the pattern of test_gpu_photometric_ext.py)"""
    lib = _lib.load()
    offs, pos = [], 64
    for k, (a, _) in enumerate(jobs):
        pos = ((pos + 3) & ~3) + misalign[k % len(misalign)]
        offs.append(pos)
        pos += a.nbytes
    buf = np.full(pos + 64, 7, np.uint8)
    for (a, _), o in zip(jobs, offs):
        buf[o:o + a.nbytes] = a.reshape(-1)
    dbuf = torch.from_numpy(buf).cuda()
    doffs, pos = [], 16
    for k, (a, _) in enumerate(jobs):
        pos = ((pos + 3) & ~3) + dst_misalign[k % len(dst_misalign)]
        doffs.append(pos)
        pos += a.nbytes + 8
    out = torch.full((pos + 16,), 7, dtype=torch.uint8, device="cuda")
    tab, descs = _tables_and_descs(jobs, offs, doffs)
    tables = torch.from_numpy(tab.view(np.int16)).cuda()
    _call(lib, dbuf.data_ptr(), dbuf.numel(), out.data_ptr(), out.numel(), descs, tables, c)
    o = out.cpu().numpy()
    written = np.zeros(o.size, bool)
    res = []
    for (a, _), p in zip(jobs, doffs):
        res.append(o[p:p + a.nbytes].reshape(a.shape))
        written[p:p + a.nbytes] = True
    assert (o[~written] == 7).all(), "bytes outside the destinations were written"
    assert np.array_equal(dbuf.cpu().numpy(), buf), "the sources were written"
    assert np.array_equal(tables.cpu().numpy().view(np.uint16), tab), "the tables were written"
    return res


def _assert_jobs(jobs, got, tag, want=None):
    for k, ((a, s), g) in enumerate(zip(jobs, got)):
        w = _want(a, s) if want is None else want[k]
        assert g.shape == w.shape and np.array_equal(g, w), (tag, k, a.shape, {n: s[n] for n in ("first", "second", "aggregation")},
                                                             [(x.shape, up) for x, up in s["grids"]], f"{int((g != w).sum())} bytes differ")


def _matrix_jobs(c):
    rng = np.random.default_rng(500 + c)
    pairs = [(f, s) for f in KINDS for s in KINDS]
    jobs, k = [], 0
    # one grid: every size x every grid shape (and one of extreme values) x every method
    for si, (w, h) in enumerate(SIZES):
        for gi, shape in enumerate(GRIDS + [GRIDS[si % len(GRIDS)]]):
            for up in (no.NEAREST, no.LINEAR, no.CUBIC):
                grids = [(_grid(rng, shape, extreme=gi == len(GRIDS)), up)]
                spec = _spec(rng, grids, pairs[k % 9], (k // 9) % 2, _curve((k // 2) % 3, rng))
                jobs.append((po.make_image(rng, h, w, c, checker=k % 5 == 0), spec))
                k += 1
    # two and three grids with mixed methods and sizes, both aggregations
    for w, h in SIZES:
        for n_it in (2, 3):
            for aggregation in (no.MAX, no.AVG):
                for _ in range(2):
                    ups = rng.permutation(3)[:n_it] if rng.random() < 0.7 else rng.integers(0, 3, n_it)
                    grids = [(_grid(rng, GRIDS[int(rng.integers(0, len(GRIDS)))], extreme=rng.random() < 0.15), int(up)) for up in ups]
                    jobs.append((po.make_image(rng, h, w, c, checker=False), _spec(rng, grids, pairs[k % 9], aggregation, _curve(k % 3, rng))))
                    k += 1
    return jobs


@pytest.mark.parametrize("c", [1, 3])
def test_equals_the_oracle_over_the_case_matrix(c):
    jobs = _matrix_jobs(c)
    # what the matrix covers
    single = [(a.shape[1], a.shape[0], s["grids"][0][0].shape, s["grids"][0][1]) for a, s in jobs if len(s["grids"]) == 1]
    assert {(w, h, up) for w, h, _, up in single} == {(w, h, up) for w, h in SIZES for up in range(3)}
    assert {(g, up) for _, _, g, up in single} == {(g, up) for g in GRIDS for up in range(3)}
    assert {(s["first"][0], s["second"][0]) for _, s in jobs} == {(f, t) for f in KINDS for t in KINDS}
    assert {(len(s["grids"]), s["aggregation"]) for _, s in jobs} >= {(n, g) for n in (1, 2, 3) for g in (no.MAX, no.AVG)}
    assert any(len({up for _, up in s["grids"]}) == 3 for _, s in jobs)
    assert any(set(np.unique(s["grids"][0][0])) <= {0, 32768} for _, s in jobs) and len(jobs) > 24
    _assert_jobs(jobs, _device(jobs, c), ("matrix", c))


def _photometric_on_device(images, fields, c):
    """ubd_photometric_images of every image with its descriptor fields (mode FILTER3 / AFFINE), dword-aligned buffers"""
    lib = _lib.load()
    offs = np.concatenate([[0], np.cumsum([(a.nbytes + 3) & ~3 for a in images])]).astype(np.int64)
    src = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for a, o in zip(images, offs):
        src[int(o):int(o) + a.nbytes] = torch.from_numpy(a.reshape(-1)).cuda()
    dst = torch.zeros_like(src)
    descs = np.zeros(len(images), aug.PHOTO_DESC)
    for k, (a, f) in enumerate(zip(images, fields)):
        descs[k]["src_offset"] = descs[k]["dst_offset"] = offs[k]
        descs[k]["w"], descs[k]["h"], descs[k]["mode"] = a.shape[1], a.shape[0], f["mode"]
        descs[k]["p"][:len(f["p"])] = f["p"]
    _lib.check(lib.ubd_photometric_images(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), descs.ctypes.data, c, len(images),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ubd_photometric_images")
    o = dst.cpu().numpy()
    return [o[int(offs[k]):int(offs[k]) + a.nbytes].reshape(a.shape) for k, a in enumerate(images)]


@pytest.mark.parametrize("c", [1, 3])
def test_known_answers(c):
    rng = np.random.default_rng(40 + c)
    ones, zeros = np.full(257, 16384), np.zeros(257, np.int64)
    images = [po.make_image(rng, h, w, c, checker=False) for w, h in SIZES]
    jobs, want = [], []

    def grids():
        return [(_grid(rng, GRIDS[int(rng.integers(0, len(GRIDS)))]), int(rng.integers(0, 3))) for _ in range(int(rng.integers(1, 4)))]
    # curve all 16384: the first branch alone = ubd_photometric_images in mode FILTER3 / AFFINE on the same image
    first = []
    for kind, mode in ((no.FILTER3, po.FILTER3), (no.AFFINE, po.AFFINE)):
        for a in images:
            br = _branch(kind, rng)
            jobs.append((a, {"first": br, "second": _branch(KINDS[int(rng.integers(0, 3))], rng), "grids": grids(), "aggregation": no.MAX, "curve": ones}))
            first.append({"mode": mode, "p": br[1]})
    want += _photometric_on_device([a for a, _ in jobs], first, c)
    # curve all 0: the second branch
    for a in images:
        s = _spec(rng, grids(), (KINDS[int(rng.integers(0, 3))], KINDS[1 + len(jobs) % 2]), no.AVG, zeros)
        jobs.append((a, s))
        want.append(no.branch(a, *s["second"]))
    # IDENTITY / IDENTITY: the source for any mask
    for a in images:
        jobs.append((a, _spec(rng, grids(), (no.IDENTITY, no.IDENTITY), int(rng.integers(0, 2)), _curve(len(jobs) % 3, rng))))
        want.append(a)
    # a constant grid with the identity curve: u = g0 for every method (the weights sum to one), a = 64 (g0 >> 7) + ((g0 & 127) + 1 >> 1)
    for k, a in enumerate(images):
        g0 = int((0, 32768, 12345, 127, 128, 16383)[k % 6])
        s = _spec(rng, [(np.full(GRIDS[k % len(GRIDS)], g0, np.uint16), k % 3)] * (1 + k % 3), (no.FILTER3, no.AFFINE), k % 2, IDENT_CURVE)
        alpha = 64 * (g0 >> 7) + (((g0 & 127) + 1) >> 1)
        f, t = no.branch(a, *s["first"]).astype(np.int64), no.branch(a, *s["second"]).astype(np.int64)
        jobs.append((a, s))
        want.append(((alpha * f + (16384 - alpha) * t + 8192) >> 14).astype(np.uint8))
    got = _device(jobs, c)
    _assert_jobs(jobs, got, ("known", c), want)
    _assert_jobs(jobs, got, ("known, oracle", c))                        # and the oracle agrees with all of them


def _mixed_jobs(rng, c, n):
    first = [(130, 33), (64, 64), (97, 35), (150, 20), (33, 70), (90, 41), (1, 9), (70, 18), (5, 5)]
    pairs = [(f, s) for f in KINDS for s in KINDS]
    jobs = []
    for k in range(n):
        w, h = first[k] if k < len(first) else (int(rng.integers(1, 150)), int(rng.integers(1, 60)))
        grids = [(_grid(rng, (int(rng.integers(1, 17)), int(rng.integers(1, 17)))), int(rng.integers(0, 3))) for _ in range(1 + k % 3)]
        jobs.append((po.make_image(rng, h, w, c), _spec(rng, grids, pairs[k % 9], k % 2, _curve(k % 3, rng))))
    return jobs


def test_one_call_over_several_launches():
    jobs = _mixed_jobs(np.random.default_rng(61), 3, 61)                 # 24 images per launch: three launches, the last one short
    _assert_jobs(jobs, _device(jobs, 3), "launches")


def test_graph_capture_replays_on_changed_source_bytes():
    lib = _lib.load()
    rng = np.random.default_rng(91)
    jobs = _mixed_jobs(rng, 3, 30)
    offs = np.concatenate([[0], np.cumsum([(a.nbytes + 3) & ~3 for a, _ in jobs])]).astype(np.int64)
    tab, descs = _tables_and_descs(jobs, offs[:-1], offs[:-1])
    tables = torch.from_numpy(tab.view(np.int16)).cuda()

    def upload(buf, js):
        for (a, _), o in zip(js, offs):
            buf[int(o):int(o) + a.nbytes] = torch.from_numpy(a.reshape(-1)).cuda()
    buf = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(buf)
    upload(buf, jobs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(lib, buf.data_ptr(), buf.numel(), out.data_ptr(), out.numel(), descs, tables, 3)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(lib, buf.data_ptr(), buf.numel(), out.data_ptr(), out.numel(), descs, tables, 3)
    for rep in range(2):
        jobs = [(po.make_image(rng, a.shape[0], a.shape[1], 3, checker=False), sp) for a, sp in jobs]      # new source bytes
        upload(buf, jobs)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _assert_jobs(jobs, [got[int(offs[k]):int(offs[k]) + a.nbytes].reshape(a.shape) for k, (a, _) in enumerate(jobs)], ("graph", rep))


def test_limits_are_refused_with_a_message():
    lib = _lib.load()
    src = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    dst = torch.full((1024,), 9, dtype=torch.uint8, device="cuda")
    tables = torch.zeros(600, dtype=torch.int16, device="cuda")

    def desc(**kw):
        d = np.zeros(1, aug.NOISE_ALPHA_DESC)
        d["w"], d["h"], d["iterations"] = 8, 8, 1
        d["grid"]["gw"], d["grid"]["gh"] = 4, 4
        d["curve_offset"] = 300
        for k, v in kw.items():
            path = k.split("__")                                         # grid__gw, first__kind, first__p__3, grid__1__upscale
            t = d
            for name in path[:-1]:
                t = t[:, int(name)] if name.isdigit() else t[name]
            if path[-1].isdigit():
                t[:, int(path[-1])] = v
            else:
                t[path[-1]] = v
        return d

    def call(d, c=3, s=None, t=None, sb=1024, db=1024, tab=None, tc=600, n=None):
        return lib.ubd_noise_alpha_images(src.data_ptr() if s is None else s, sb, dst.data_ptr() if t is None else t, db,
                                          d.ctypes.data if d is not None else None, tables.data_ptr() if tab is None else tab, tc, c,
                                          len(d) if n is None else n, None)
    F3, AF = no.FILTER3, no.AFFINE
    good = [dict(d=desc()), dict(d=desc(iterations=3, aggregation=1), c=1), dict(d=desc(grid__gw=16, grid__gh=16, grid__upscale=2)),
            dict(d=desc(first__kind=F3, first__p__0=13 * 16384, first__p__8=-13 * 16384)), dict(d=desc(second__kind=AF, second__p__2=1 << 17, second__p__5=-(1 << 24))),
            dict(d=desc(curve_offset=343, grid__0__grid_offset=584)),                          # both end exactly at table_count
            dict(d=desc(first__kind=F3), s=dst.data_ptr(), sb=512, t=dst.data_ptr() + 512, db=512)]   # disjoint ranges of one buffer
    for kw in good:
        assert call(**kw) == 0, (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    dst.fill_(9)
    torch.cuda.synchronize()
    bad = [dict(d=desc(iterations=0)), dict(d=desc(iterations=4)), dict(d=desc(iterations=-1))]
    bad += [dict(d=desc(**{f"grid__{name}": v})) for name in ("gw", "gh") for v in (0, 17, -1)]
    bad += [dict(d=desc(iterations=2, grid__1__gw=17)), dict(d=desc(iterations=3, grid__2__upscale=3))]
    bad += [dict(d=desc(grid__upscale=v)) for v in (3, -1)] + [dict(d=desc(aggregation=v)) for v in (2, -1)]
    bad += [dict(d=desc(**{f"{br}__kind": v})) for br in ("first", "second") for v in (3, -1, 16)]
    bad += [dict(d=desc(first__kind=F3, first__p__4=13 * 16384 + 1)), dict(d=desc(second__kind=F3, second__p__8=-13 * 16384 - 1)),
            dict(d=desc(first__kind=AF, first__p__0=(1 << 17) + 1)), dict(d=desc(first__kind=AF, first__p__2=-(1 << 17) - 1)),
            dict(d=desc(second__kind=AF, second__p__3=(1 << 24) + 1)), dict(d=desc(second__kind=AF, second__p__5=-(1 << 24) - 1))]
    bad += [dict(d=desc(curve_offset=344)), dict(d=desc(curve_offset=-1)), dict(d=desc(curve_offset=1 << 40)),
            dict(d=desc(grid__0__grid_offset=585)), dict(d=desc(grid__0__grid_offset=-1)), dict(d=desc(iterations=2, grid__1__grid_offset=600)),
            dict(d=desc(), tc=556), dict(d=desc(), tc=0)]
    bad += [dict(d=desc(), c=2), dict(d=desc(), c=0), dict(d=desc(w=0)), dict(d=desc(w=16385)), dict(d=desc(h=0)), dict(d=desc(h=16385)),
            dict(d=desc(), n=0), dict(d=desc(), n=-1), dict(d=desc(), s=0), dict(d=desc(), t=0), dict(d=desc(), tab=0), dict(d=None, n=1),
            dict(d=desc(src_offset=1024 - 191)), dict(d=desc(dst_offset=1024 - 191)), dict(d=desc(src_offset=-1))]
    # every overlap of source and destination, the same range included
    bad += [dict(d=desc(), s=dst.data_ptr()), dict(d=desc(dst_offset=32), s=dst.data_ptr()), dict(d=desc(dst_offset=191), s=dst.data_ptr()),
            dict(d=desc(), s=dst.data_ptr(), sb=512, t=dst.data_ptr() + 191, db=512), dict(d=desc(src_offset=100), s=dst.data_ptr())]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.ubd_last_error().decode().startswith("ubd_noise_alpha_images"), (kw, lib.ubd_last_error())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 9).all()                                # nothing was launched for a refused call
    assert lib.ubd_abi_version() == 3


# ---------------------------------------------------------------------------------------------------------------- the chain
def _pillow_chain(im, plan):
    for st in plan.stages:
        if st.kind in ("rotate", "quarter"):
            im = im.rotate(st.params["angle"], Image.BILINEAR, expand=True)
        elif st.kind == "crop":
            im = im.crop(st.params["box"])
        else:
            im = im.transform(im.size, Image.PERSPECTIVE, st.params["coeffs"], Image.BILINEAR)
    return im


def _pil(a):
    return Image.fromarray(a[..., 0] if a.shape[2] == 1 else a, "L" if a.shape[2] == 1 else "RGB")


def _arr(im):
    r = np.asarray(im)
    return r[..., None] if r.ndim == 2 else r


def _na_kinds(plan):
    return set() if plan.original else {st.kind for st in plan.photometric if st.kind in aug.NOISE_ALPHA_KINDS}


def _chain_cases(size=(90, 60)):
    """seeded (image, plan) pairs on 90 x 60 images whose photometric plans hold each mask-blended kind at least twice, in
    different slots; plans with a NOISE stage (fp32 transcendentals: it would need the margin rule of
    tests/test_gpu_photometric.py) are passed over"""
    mk = [ObjectMarkup([30, 20, 60, 20, 60, 40, 30, 40])]
    rs = np.random.default_rng(12)
    need = {(k, n) for k in aug.NOISE_ALPHA_KINDS for n in range(2)}
    slots = {k: set() for k in aug.NOISE_ALPHA_KINDS}
    out = []
    for seed in range(5000):
        if not need:
            break
        plan = aug.sample_plan(size, mk, random.Random(seed), np.random.RandomState(seed), np.random.default_rng(seed), photo_extended=True,
                               photo_noise_alpha=True)
        if plan.original or any(st.kind == "noise" for st in plan.photometric):
            continue
        assert not any(st.kind == "unbuilt" for st in plan.photometric)
        add = set()
        for i, st in enumerate(plan.photometric):
            if st.kind in aug.NOISE_ALPHA_KINDS and i not in slots[st.kind] and (st.kind, len(slots[st.kind])) in need:
                add.add((st.kind, len(slots[st.kind])))
                slots[st.kind].add(i)
        if add:
            need -= add
            out.append((rs.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8), plan))
    assert not need, need
    return out


def _assert_chain(got, a, plan, tag):
    c = a.shape[2]
    ref = _arr(_pillow_chain(_pil(a), plan))
    for st in () if plan.original else plan.photometric:
        if st.kind in aug.NOISE_ALPHA_KINDS:
            ref = no.apply_fields(ref, *aug.noise_alpha_descs(st, ref.shape[1], ref.shape[0], c))
            continue
        f = aug.photometric_descs(st, ref.shape[1], ref.shape[0], c)
        if f is not None:
            assert f["mode"] != po.NOISE
            ref = (pe if f["mode"] >= pe.MEDIAN else po).apply(ref, f["mode"], f["p"], f["flags"], f["seed"])
    assert got.shape == ref.shape and np.array_equal(got, ref), (tag, plan, f"{int((got != ref).sum())} bytes differ")


def test_device_chain_equals_pillow_then_the_oracles():
    cases = _chain_cases()
    assert set().union(*(_na_kinds(p) for _, p in cases)) == set(aug.NOISE_ALPHA_KINDS)
    got = aug.augment_arrays_on_device([a for a, _ in cases], [p for _, p in cases])
    for k, ((a, plan), g) in enumerate(zip(cases, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("rgb", k))
    # grey images, sources on the device, read in place and never written
    greys = [np.ascontiguousarray(a[:, :, 1:2]) for a, _ in cases]
    tensors = [torch.from_numpy(a).cuda() for a in greys]
    got = aug.augment_arrays_on_device(tensors, [p for _, p in cases])
    for k, (a, (_, plan), t, g) in enumerate(zip(greys, cases, tensors, got)):
        _assert_chain(g.cpu().numpy(), a, plan, ("grey", k))
        assert np.array_equal(t.cpu().numpy(), a)
    # a caller's tensor whose only stage is a mask-blended one: it goes to a new buffer, a pointwise stage after it runs in place
    a = cases[0][0]
    st = next(s for _, p in cases for s in p.photometric if s.kind == "frequency_alpha")
    plan = aug.AugmentationPlan((90, 60), (), False, True, (st, aug.Stage("add", {"values": (5, -7, 9), "per_channel": True, "entry": 7}, None)))
    t = torch.from_numpy(a).cuda()
    g = aug.augment_arrays_on_device([t], [plan])[0]
    assert np.array_equal(t.cpu().numpy(), a) and g.data_ptr() != t.data_ptr()
    _assert_chain(g.cpu().numpy(), a, plan, "owned")


def test_prepare_batches_runs_the_whole_stage():
    cfg = NetConfig(grey=False)
    rs = np.random.default_rng(18)
    frames, markups = [], []
    for k in range(8):
        h, w = int(rs.integers(60, 96)), int(rs.integers(60, 96))
        frames.append(rs.integers(0, 256, (h, w, 3), dtype=np.uint8))
        markups.append([ObjectMarkup(q.reshape(-1).tolist()) for q in synthetic.random_quads(rs, h, w, 1, 2, 12, 30)])

    def plans_of(seed):
        g, r, n = np.random.default_rng(seed), random.Random(seed), np.random.RandomState(seed)
        return [aug.sample_plan((a.shape[1], a.shape[0]), m, r, n, g, True, True) for a, m in zip(frames, markups)]
    for seed in range(2000):                                             # found on the CPU: both kinds occur, no NOISE stage
        want = plans_of(seed)
        if set().union(*(_na_kinds(p) for p in want)) == set(aug.NOISE_ALPHA_KINDS) and not any(st.kind == "noise" for p in want for st in p.photometric):
            break
    else:
        raise AssertionError("no seed found")
    random.seed(seed)
    np.random.seed(seed)
    groups = SegmapManager.prepare_batches_on_device(frames, markups, cfg, augment=True, photo_rng=np.random.default_rng(seed),
                                                     photo_extended=True, photo_noise_alpha=True)
    plans = {i: p for idx, _, _, _, ps in groups for i, p in zip(idx, ps)}
    images = {i: x.cpu().numpy()[j] for idx, x, _, _, _ in groups for j, i in enumerate(idx)}
    assert [plans[i] for i in range(len(frames))] == want
    assert not any(st.kind == "unbuilt" for p in want for st in p.photometric)
    # the images with a mask-blended stage are the oracles' stages on Pillow's chain, rescaled like the others
    warped = aug.augment_arrays_on_device(frames, want)
    for k, p in enumerate(want):
        if _na_kinds(p):
            _assert_chain(warped[k].cpu().numpy(), frames[k], p, ("batch", k))
            im, _ = SegmapManager._rescale_image_and_markup(_pil(warped[k].cpu().numpy()), aug.apply_plan_to_markup(p, markups[k]), cfg)
            assert np.array_equal(images[k], _arr(im))
