"""CPU: the n-edge scan line of ubdvss_amd/csrc/polygon_fill.h, built for the host, against Pillow itself.

polygon_fill.h states ImageDraw.polygon's fill rule for a polygon of up to 64 vertices as steps that are each one edge's work
(raster.hip gives them to the lanes of a wave) and strings them together sequentially in pf_row_spans.  The header is plain C++
apart from the device qualifiers and five rounding intrinsics, so a small program with those defined away compiles it with the
host compiler (-ffp-contract=off, as the device unit is built).  Required, with 0 differing pixels, against the installed Pillow
and against oracle/label_raster.py's fill_polygon:
  * strictly convex hulls of random integer point clouds, 3..64 vertices, both windings, every start vertex, partly off the
    canvas, canvases 8..80 wide;
  * hulls of rasterised shapes after the reference's rescale, the division by the map scale 4 and the truncation
    (segmap_manager.py:114-116; the program divides and truncates with pf_truncate);
  * polygons with repeated consecutive vertices.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageDraw

from oracle import label_raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#define __device__
#define __forceinline__ inline
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
static inline double __ddiv_rn(double a, double b) { volatile double r = a / b; return r; }
#include "polygon_fill.h"
// argv: polygons file (text, per polygon: h w scale n, then 2n doubles), output file: per polygon h * w bytes of 0 / 1
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int h, w, scale, n;
    while (fscanf(in, "%d %d %d %d", &h, &w, &scale, &n) == 4) {
        if (n < 1 || n > PF_MAX_VERTS) return 4;
        int vx[PF_MAX_VERTS], vy[PF_MAX_VERTS], spans[2 * (2 * PF_MAX_VERTS)];
        for (int i = 0; i < n; ++i) {
            double x, y;
            if (fscanf(in, "%lf %lf", &x, &y) != 2) return 5;
            vx[i] = pf_truncate(x, scale); vy[i] = pf_truncate(y, scale);
        }
        std::vector<unsigned char> img((size_t)h * w, 0);
        for (int y = 0; y < h; ++y) {
            const int ns = pf_row_spans(vx, vy, n, y, h, spans);
            for (int s = 0; s < ns; ++s)
                for (int x = std::max(spans[2 * s], 0); x <= std::min(spans[2 * s + 1], w - 1); ++x) img[(size_t)y * w + x] = 1;
        }
        fwrite(img.data(), 1, img.size(), out);
    }
    fclose(out);
    return 0;
}
"""


def strict_hull(points):
    """strictly convex hull of integer points (monotone chain), counter-clockwise in x right / y up terms"""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) < 3:
        return pts

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = half(pts), half(reversed(pts))
    return lower[:-1] + upper[:-1]


def cloud_hulls(rng, count):
    """(h, w, hull) with 3..64 vertices: uniform clouds (few vertices) and rounded rings of radius up to 110 (many), centred
    anywhere near the canvas so that most lie partly off it"""
    out = []
    while len(out) < count:
        w, h = int(rng.integers(8, 81)), int(rng.integers(8, 81))
        if len(out) % 2:
            k = 3 if len(out) % 10 == 1 else int(rng.integers(3, 40))          # triangles among them
            pts = np.stack([rng.integers(-10, w + 10, k), rng.integers(-10, h + 10, k)], axis=1)
        else:
            ra, rb = rng.uniform(3, 110, 2)
            cx, cy = rng.uniform(-20, w + 20), rng.uniform(-20, h + 20)
            t = rng.uniform(0, 2 * np.pi, int(rng.integers(8, 400)))
            pts = np.round(np.stack([cx + ra * np.cos(t), cy + rb * np.sin(t)], axis=1)).astype(int)
        hull = strict_hull(pts)
        if 3 <= len(hull) <= 64:
            out.append((h, w, hull))
    return out


def shape_hulls(rng, count):
    """hulls of rasterised rotated rectangles and ellipses on a 128 x 160 map, as float markup rescaled to 136 x 152"""
    H, W = 128, 160
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    while len(out) < count:
        cx, cy = rng.uniform(10, W - 10), rng.uniform(10, H - 10)
        a, b = rng.uniform(3, 60), rng.uniform(3, 40)
        ang = rng.uniform(0, np.pi)
        u = (xs - cx) * np.cos(ang) + (ys - cy) * np.sin(ang)
        v = -(xs - cx) * np.sin(ang) + (ys - cy) * np.cos(ang)
        mask = (np.abs(u) <= a) & (np.abs(v) <= b) if len(out) % 2 else (u / a) ** 2 + (v / b) ** 2 <= 1
        py, px = np.nonzero(mask)
        hull = strict_hull(zip(px, py))
        if 3 <= len(hull) <= 64:
            factors = np.array([[152 / W, 136 / H]])
            out.append((136 // 4, 152 // 4, (np.array(hull, np.float64) * factors).tolist()))
    return out


def pillow(h, w, ipts):
    im = Image.new('L', (w, h), 0)
    ImageDraw.Draw(im).polygon([int(v) for v in ipts], fill=1)
    return np.asarray(im) > 0


def mirror(h, w, ipts):
    m = np.zeros((h, w), np.int32)
    label_raster.fill_polygon(m, [int(v) for v in ipts], 1)
    return m > 0


@pytest.fixture(scope="module")
def host_fill(tmp_path_factory):
    """runs the host build of polygon_fill.h on a list of (h, w, scale, vertices); returns the list of boolean masks"""
    work = tmp_path_factory.mktemp("polygon_fill")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "a host C++ compiler is needed to build polygon_fill.h for the CPU"
    (work / "fill.cpp").write_text(PROGRAM)
    subprocess.check_call([compiler, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ubdvss_amd", "csrc"),
                           "-o", str(work / "fill"), str(work / "fill.cpp")])

    def run(cases):
        lines = [f"{h} {w} {s} {len(p)} " + " ".join(f"{float(x)!r} {float(y)!r}" for x, y in p) for h, w, s, p in cases]
        (work / "polys.txt").write_text("\n".join(lines) + "\n")
        subprocess.check_call([str(work / "fill"), str(work / "polys.txt"), str(work / "masks.bin")])
        raw = np.fromfile(str(work / "masks.bin"), np.uint8)
        out, at = [], 0
        for h, w, _, _ in cases:
            out.append(raw[at:at + h * w].reshape(h, w) > 0)
            at += h * w
        assert at == raw.size
        return out
    return run


def _variants(hull):
    """every start vertex, both windings"""
    for seq in (hull, hull[::-1]):
        for s in range(len(seq)):
            yield seq[s:] + seq[:s]


def _compare(host_fill, cases, with_mirror=True):
    masks = host_fill(cases)
    bad_pillow, bad_mirror = [], []
    for (h, w, s, p), m in zip(cases, masks):
        ipts = (np.asarray(p, np.float64) / s).astype(np.int32).reshape(-1)         # segmap_manager.py:114-116
        if not np.array_equal(m, pillow(h, w, ipts)):
            bad_pillow.append((h, w, ipts.tolist()))
        if with_mirror and not np.array_equal(m, mirror(h, w, ipts)):
            bad_mirror.append((h, w, ipts.tolist()))
    assert not bad_pillow, f"{len(bad_pillow)} of {len(cases)} differ from Pillow, first {bad_pillow[0]}"
    assert not bad_mirror, f"{len(bad_mirror)} of {len(cases)} differ from fill_polygon, first {bad_mirror[0]}"
    return masks


def test_hulls_of_integer_clouds_equal_pillow_for_every_start_vertex_and_winding(host_fill):
    hulls = cloud_hulls(np.random.default_rng(11), 50)
    sizes = sorted(len(p) for _, _, p in hulls)
    assert sizes[0] == 3 and sizes[-1] >= 48, sizes
    cases = [(h, w, 1, v) for h, w, hull in hulls for v in _variants(hull)]
    masks = _compare(host_fill, cases, with_mirror=False)
    assert sum(m.any() for m in masks) > len(masks) // 2
    # the sequential statement is slow: one winding and three start vertices of every hull
    _compare(host_fill, [(h, w, 1, v) for h, w, hull in hulls for k, v in enumerate(_variants(hull)) if k % max(1, len(hull) // 3) == 0])


def test_an_exact_64_vertex_hull(host_fill):
    """the limit itself: 64 rounded points of an ellipse that are all hull vertices"""
    pts = [(int(round(-350 + 420 * np.cos(a))), int(round(36 + 380 * np.sin(a)))) for a in np.linspace(0.01, 2 * np.pi + 0.01, 64, endpoint=False)]
    hull = strict_hull(pts)
    assert len(hull) == 64
    _compare(host_fill, [(72, 80, 1, v) for k, v in enumerate(_variants(hull)) if k % 8 == 0])


def test_rasterised_shape_hulls_after_rescale_division_and_truncation(host_fill):
    shapes = shape_hulls(np.random.default_rng(12), 200)
    assert max(len(p) for _, _, p in shapes) >= 24
    cases = [(h, w, 4, p) for h, w, p in shapes] + [(h, w, 4, p[::-1]) for h, w, p in shapes[:100]]
    _compare(host_fill, cases)


def test_repeated_consecutive_vertices(host_fill):
    rng = np.random.default_rng(13)
    cases = []
    for h, w, hull in cloud_hulls(rng, 150):
        if len(hull) > 40:
            continue
        reps = rng.integers(1, 3, len(hull))
        doubled = [p for p, r in zip(hull, reps) for _ in range(r)]
        shift = int(rng.integers(0, len(doubled)))
        cases.append((h, w, 1, doubled[shift:] + doubled[:shift]))
    assert len(cases) > 80
    _compare(host_fill, cases)
