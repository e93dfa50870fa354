"""CPU: the two statements of the polygon fill rule in ubdvss_amd/csrc/raster_fill.h, built for the host.

raster_fill.h holds rq_covers (one pixel; the text raster.hip has always compiled) and rq_covers_run (a run of adjacent pixels
from one evaluation of the scan line; visualize.hip).  The header is plain C++ apart from the device qualifiers and four
rounding intrinsics, so a small program with those defined away compiles it with the host compiler (-ffp-contract=off, as
the device units are built) and this test checks, on random quads:
  * rq_covers_run gives the bits of rq_covers, for runs of four pixels and a ragged last run;
  * no covered pixel lies outside the row / column extent of the four corners (visualize.hip skips quads on that ground);
  * rq_covers equals oracle/label_raster.py's fill_polygon, the sequential statement pinned to Pillow;
  * on convex quads (what the postprocess finds) the rule equals Pillow itself;
  * the one known self-intersecting sliver on which the rule and Pillow differ, by exactly one pixel.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageDraw

from oracle import label_raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 45                                   # odd sizes: the last run of a row has one pixel

PROGRAM = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#define __device__
#define __forceinline__ inline
using std::max; using std::min;
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
#include "raster_fill.h"
// argv: quads file (text: H W count, then 8 integers per quad), output file: per quad H * W bytes, bit 0 = rq_covers, bit 1 = rq_covers_run
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "wb");
    int h, w, count;
    if (!in || !out || fscanf(in, "%d %d %d", &h, &w, &count) != 3) return 3;
    for (int q = 0; q < count; ++q) {
        int p[8];
        for (int j = 0; j < 8; ++j) if (fscanf(in, "%d", &p[j]) != 1) return 4;
        for (int y = 0; y < h; ++y)
            for (int x0 = 0; x0 < w; x0 += 4) {
                const int npx = min(4, w - x0);
                const unsigned run = rq_covers_run(p, x0, npx, y, h);
                for (int k = 0; k < npx; ++k) fputc((rq_covers(p, x0 + k, y, h) ? 1 : 0) | (((run >> k) & 1u) ? 2 : 0), out);
            }
    }
    fclose(out);
    return 0;
}
"""


def _opposite_corners_coincide(q):
    return (q[0] == q[4] and q[1] == q[5]) or (q[2] == q[6] and q[3] == q[7])


def _arbitrary_quads(rng, count):
    """corners in any order: convex, concave and self-intersecting outlines, inside, partly outside and far outside the canvas"""
    out = []
    while len(out) < count:
        kind = len(out) % 4
        if kind == 0:
            q = rng.integers(-10, 60, 8)
        elif kind == 1:
            q = rng.integers(0, 12, 8) + rng.integers(0, 30)            # small: slivers, repeated rows and columns
        elif kind == 2:
            x0, y0 = rng.integers(-5, 40, 2)
            bw, bh = rng.integers(0, 20, 2)
            q = np.array([x0, y0, x0 + bw, y0, x0 + bw, y0 + bh, x0, y0 + bh])
        else:
            q = rng.integers(-40, 90, 8)
        if not _opposite_corners_coincide(q):                           # raster.hip's documented exception
            out.append([int(v) for v in q])
    return out


def _convex_quads(rng, count):
    """rotated rectangles with rounded corners, kept when still convex with non-zero area: the boxes a postprocess finds"""
    out = []
    while len(out) < count:
        a, b = rng.uniform(1, 30, 2)
        ang = rng.uniform(0, np.pi)
        cx, cy = rng.uniform(-5, W + 5), rng.uniform(-5, H + 5)
        ca, sa = np.cos(ang), np.sin(ang)
        pts = np.array([[cx + dx * ca - dy * sa, cy + dx * sa + dy * ca] for dx, dy in ((-a, -b), (a, -b), (a, b), (-a, b))])
        p = np.round(pts / 2 + np.array([cx, cy]) / 2).astype(int)
        e = np.roll(p, -1, axis=0) - p
        cross = e[:, 0] * np.roll(e[:, 1], -1) - e[:, 1] * np.roll(e[:, 0], -1)
        if (cross > 0).all() or (cross < 0).all():
            out.append([int(v) for v in p.reshape(-1)])
    return out


def _pillow(q):
    im = Image.new('L', (W, H), 0)
    ImageDraw.Draw(im).polygon(q, fill=255)
    return np.asarray(im) > 0


def _mirror(q):
    m = np.zeros((H, W), np.int32)
    label_raster.fill_polygon(m, q, 1)
    return m > 0


KNOWN_SLIVER = [23, 17, 16, 19, 25, 17, 19, 18]


@pytest.fixture(scope="module")
def host_fill(tmp_path_factory):
    """runs the host build of raster_fill.h on a list of quads; returns (single, run) boolean masks (count, H, W)"""
    work = tmp_path_factory.mktemp("raster_fill")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "a host C++ compiler is needed to build raster_fill.h for the CPU"
    (work / "fill.cpp").write_text(PROGRAM)
    subprocess.check_call([compiler, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ubdvss_amd", "csrc"),
                           "-o", str(work / "fill"), str(work / "fill.cpp")])

    def run(quads):
        (work / "quads.txt").write_text(f"{H} {W} {len(quads)}\n" + "\n".join(" ".join(str(v) for v in q) for q in quads) + "\n")
        subprocess.check_call([str(work / "fill"), str(work / "quads.txt"), str(work / "masks.bin")])
        raw = np.fromfile(str(work / "masks.bin"), np.uint8).reshape(len(quads), H, W)
        return (raw & 1) > 0, (raw & 2) > 0
    return run


def test_run_form_equals_the_one_pixel_form_and_stays_inside_the_corner_extent(host_fill):
    quads = _arbitrary_quads(np.random.default_rng(1), 3000) + _convex_quads(np.random.default_rng(2), 1000) + [KNOWN_SLIVER]
    single, run = host_fill(quads)
    assert single.any(axis=(1, 2)).sum() > 3000
    assert np.array_equal(single, run), f"{int((single != run).any(axis=(1, 2)).sum())} quads differ between rq_covers and rq_covers_run"
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for q, m in zip(quads, single):
        inside = (xs >= min(q[0::2])) & (xs <= max(q[0::2])) & (ys >= min(q[1::2])) & (ys <= max(q[1::2]))
        assert not (m & ~inside).any(), q


def test_one_pixel_form_equals_the_sequential_statement(host_fill):
    quads = _arbitrary_quads(np.random.default_rng(3), 600) + [KNOWN_SLIVER]
    single, _ = host_fill(quads)
    for q, m in zip(quads, single):
        assert np.array_equal(m, _mirror(q)), q


def test_convex_quads_equal_pillow(host_fill):
    quads = _convex_quads(np.random.default_rng(4), 2000)
    single, run = host_fill(quads)
    differing = [q for q, m in zip(quads, single) if not np.array_equal(m, _pillow(q))]
    assert not differing, differing[:3]
    assert np.array_equal(single, run)


def test_the_known_sliver_differs_from_pillow_by_one_pixel(host_fill):
    """Documents the difference raster_fill.h and include/ubd.h record: a self-intersecting sliver, three rows high with two of
    its corners in the top row.  The rule leaves pixel (22, 17) unset; Pillow sets it."""
    single, run = host_fill([KNOWN_SLIVER])
    want = _pillow(KNOWN_SLIVER)
    assert np.array_equal(single, run)
    assert np.argwhere(single[0] != want).tolist() == [[17, 22]] and want[17, 22] and not single[0, 17, 22]
