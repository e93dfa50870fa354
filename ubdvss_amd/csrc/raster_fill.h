// Pillow's ImageDraw.polygon fill rule for integer quadrilaterals, as device functions: the rule raster.hip documents (float32
// scan-line intersections, product and sum rounded separately, spans [round-half-up(left), round-half-down(right)], horizontal
// edges drawn as they are, top / bottom corner pixels joined to the neighbouring row's span) and oracle/label_raster.py pins
// against the installed Pillow.  Shared by raster.hip (training label maps) and visualize.hip (found boxes drawn at image
// resolution).  Every unit that includes this is built with -ffp-contract=off.
//
// Two statements of the one rule: rq_covers answers one pixel and is the text raster.hip has always compiled (kept word for word,
// so build_label_maps_kernel's code does not change); rq_covers_run answers a run of adjacent pixels of a row from one evaluation
// of the scan line.  tests/test_raster_fill_host.py builds both for the host and requires the same bits from them on random
// quads (convex, concave, self-intersecting, partly and wholly outside the canvas), and that no covered pixel lies outside the
// row / column extent of the four corners -- visualize.hip skips a quad on that ground.
//
// Known differences from Pillow.  (1) A quad whose opposite corners coincide (raster.hip's header).  (2) Self-intersecting
// slivers: (23,17) (16,19) (25,17) (19,18) -- three rows high, two corners in its top row, the outline crossing itself there --
// leaves pixel (22, 17) unset where Pillow 12 sets it; 1 of about 20 000 random quads in a fuzz over arbitrary corner orders, none
// among convex quads.  The boxes ubd_postprocess finds (minAreaRect rectangles) are convex.  The host test pins this example.
#pragma once

struct rq_edge { int x0, y0, x1, y1, xmin, xmax, ymin, ymax; float dx; bool horiz; };

__device__ __forceinline__ int rq_round_up(float f) { return f >= 0.f ? (int)floorf(__fadd_rn(f, 0.5f)) : -(int)floorf(__fadd_rn(fabsf(f), 0.5f)); }
__device__ __forceinline__ int rq_round_down(float f) { return f >= 0.f ? (int)ceilf(__fsub_rn(f, 0.5f)) : -(int)ceilf(__fsub_rn(fabsf(f), 0.5f)); }
__device__ __forceinline__ float rq_x_at(const rq_edge &e, int y) { return __fadd_rn(__fmul_rn((float)(y - e.y0), e.dx), (float)e.x0); }

// bits lo - px .. hi - px of a run of npx pixels that starts at px, for the part of [lo, hi] inside the run
__device__ __forceinline__ unsigned rq_run_bits(int lo, int hi, int px, int npx)
{
    lo = max(lo, px); hi = min(hi, px + npx - 1);
    return lo <= hi ? ((2u << (hi - lo)) - 1u) << (lo - px) : 0u;
}

// Which of the pixels (px .. px + npx - 1, py), npx <= 32, are inside ImageDraw.polygon(pts) on a canvas of map_h rows?  Bit k is
// pixel px + k.  One scan line of Pillow's polygon fill (oracle/label_raster.py fill_polygon is the sequential statement of the
// same rule); the scan line is worked out once for the whole run.
__device__ unsigned rq_covers_run(const int *pts, int px, int npx, int py, int map_h)
{
    rq_edge e[4];
    unsigned covered = 0u;
    int ymin = map_h - 1, ymax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rq_edge &d = e[i];
        d.x0 = pts[2 * i]; d.y0 = pts[2 * i + 1]; d.x1 = pts[(2 * i + 2) & 7]; d.y1 = pts[(2 * i + 3) & 7];
        d.xmin = min(d.x0, d.x1); d.xmax = max(d.x0, d.x1); d.ymin = min(d.y0, d.y1); d.ymax = max(d.y0, d.y1);
        d.horiz = d.y0 == d.y1;
        d.dx = d.horiz ? 0.f : __fdiv_rn((float)(d.x1 - d.x0), (float)(d.y1 - d.y0));
        ymin = min(ymin, d.ymin); ymax = max(ymax, d.ymax);
        if (d.horiz && py == d.y0) covered |= rq_run_bits(d.xmin, d.xmax, px, npx);   // horizontal edges are drawn as they are
    }
    ymin = max(ymin, 0); ymax = min(ymax, map_h);
    if (py < ymin || py > ymax) return covered;
    // intersections of this scan line in edge order; an edge's lower end point counts twice (except in the last row)
    float xx[8];
    int last[4], act[4], na = 0, nx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (e[i].horiz || py < e[i].ymin || py > e[i].ymax) continue;
        const float x = rq_x_at(e[i], py);
        xx[nx++] = x;
        if (py == e[i].ymax && py < ymax) xx[nx++] = x;
        act[na] = i; last[na] = nx - 1; ++na;
    }
    // "connect discontiguous corners": two edges leaning to the same side that both start in one point of this row (in the
    // last row: both end there) -- the later edge's intersection moves towards the span of the neighbouring row
    for (int bi = 1; bi < na; ++bi) {
        const rq_edge &b = e[act[bi]];
        if (b.dx == 0.f) continue;
        const int bex = b.y0 == py ? b.x0 : b.x1, bey = b.y0 == py ? b.y0 : b.y1;
        for (int ai = 0; ai < bi; ++ai) {
            const rq_edge &a = e[act[ai]];
            if ((b.dx > 0.f && a.dx <= 0.f) || (b.dx < 0.f && a.dx >= 0.f)) continue;
            const bool top = a.ymin == py && b.ymin == py && py < ymax;
            const bool bottom = a.ymax == py && b.ymax == py && py == ymax;
            if (top == bottom) continue;
            const int aex = a.y0 == py ? a.x0 : a.x1, aey = a.y0 == py ? a.y0 : a.y1;
            if (aex != bex || aey != bey) continue;
            const float v = (float)aex;
            const int ya = top ? py + 1 : py - 1;
            const float xa = rq_x_at(a, ya), xb = rq_x_at(b, ya);
            const float lo = fminf(xa, xb), hi = fmaxf(xa, xb);
            if (lo > v) xx[last[bi]] = fmaxf(v, (float)(rq_round_up(lo) - 1));
            else if (hi < v) xx[last[bi]] = fminf(v, __fadd_rn(hi, 1.f));
            break;
        }
    }
    for (int a = 1; a < nx; ++a) {                                   // insertion sort, nx <= 8
        const float v = xx[a];
        int b = a - 1;
        while (b >= 0 && xx[b] > v) { xx[b + 1] = xx[b]; --b; }
        xx[b + 1] = v;
    }
    int x_pos = nx ? (int)xx[0] : 0;
    for (int i = 1; i < nx; i += 2) {
        const int x_end = rq_round_down(xx[i]);
        if (x_end < x_pos) continue;
        int x_start = rq_round_up(xx[i - 1]);
        if (x_pos > x_start) { x_start = x_pos; if (x_end < x_start) continue; }
        if (x_start > x_end) continue;
        covered |= rq_run_bits(x_start, x_end, px, npx);
        x_pos = x_end + 1;
    }
    return covered;
}

// Is pixel (px, py) inside ImageDraw.polygon(pts) on a canvas of map_h rows?  One scan line of Pillow's polygon fill
// (oracle/label_raster.py fill_polygon is the sequential statement of the same rule).
__device__ bool rq_covers(const int *pts, int px, int py, int map_h)
{
    rq_edge e[4];
    int ymin = map_h - 1, ymax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rq_edge &d = e[i];
        d.x0 = pts[2 * i]; d.y0 = pts[2 * i + 1]; d.x1 = pts[(2 * i + 2) & 7]; d.y1 = pts[(2 * i + 3) & 7];
        d.xmin = min(d.x0, d.x1); d.xmax = max(d.x0, d.x1); d.ymin = min(d.y0, d.y1); d.ymax = max(d.y0, d.y1);
        d.horiz = d.y0 == d.y1;
        d.dx = d.horiz ? 0.f : __fdiv_rn((float)(d.x1 - d.x0), (float)(d.y1 - d.y0));
        ymin = min(ymin, d.ymin); ymax = max(ymax, d.ymax);
        if (d.horiz && py == d.y0 && px >= d.xmin && px <= d.xmax) return true;       // horizontal edges are drawn as they are
    }
    ymin = max(ymin, 0); ymax = min(ymax, map_h);
    if (py < ymin || py > ymax) return false;
    // intersections of this scan line in edge order; an edge's lower end point counts twice (except in the last row)
    float xx[8];
    int last[4], act[4], na = 0, nx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (e[i].horiz || py < e[i].ymin || py > e[i].ymax) continue;
        const float x = rq_x_at(e[i], py);
        xx[nx++] = x;
        if (py == e[i].ymax && py < ymax) xx[nx++] = x;
        act[na] = i; last[na] = nx - 1; ++na;
    }
    // "connect discontiguous corners": two edges leaning to the same side that both start in one point of this row (in the
    // last row: both end there) -- the later edge's intersection moves towards the span of the neighbouring row
    for (int bi = 1; bi < na; ++bi) {
        const rq_edge &b = e[act[bi]];
        if (b.dx == 0.f) continue;
        const int bex = b.y0 == py ? b.x0 : b.x1, bey = b.y0 == py ? b.y0 : b.y1;
        for (int ai = 0; ai < bi; ++ai) {
            const rq_edge &a = e[act[ai]];
            if ((b.dx > 0.f && a.dx <= 0.f) || (b.dx < 0.f && a.dx >= 0.f)) continue;
            const bool top = a.ymin == py && b.ymin == py && py < ymax;
            const bool bottom = a.ymax == py && b.ymax == py && py == ymax;
            if (top == bottom) continue;
            const int aex = a.y0 == py ? a.x0 : a.x1, aey = a.y0 == py ? a.y0 : a.y1;
            if (aex != bex || aey != bey) continue;
            const float v = (float)aex;
            const int ya = top ? py + 1 : py - 1;
            const float xa = rq_x_at(a, ya), xb = rq_x_at(b, ya);
            const float lo = fminf(xa, xb), hi = fmaxf(xa, xb);
            if (lo > v) xx[last[bi]] = fmaxf(v, (float)(rq_round_up(lo) - 1));
            else if (hi < v) xx[last[bi]] = fminf(v, __fadd_rn(hi, 1.f));
            break;
        }
    }
    for (int a = 1; a < nx; ++a) {                                   // insertion sort, nx <= 8
        const float v = xx[a];
        int b = a - 1;
        while (b >= 0 && xx[b] > v) { xx[b + 1] = xx[b]; --b; }
        xx[b + 1] = v;
    }
    int x_pos = nx ? (int)xx[0] : 0;
    for (int i = 1; i < nx; i += 2) {
        const int x_end = rq_round_down(xx[i]);
        if (x_end < x_pos) continue;
        int x_start = rq_round_up(xx[i - 1]);
        if (x_pos > x_start) { x_start = x_pos; if (x_end < x_start) continue; }
        if (x_start > x_end) continue;
        if (px >= x_start && px <= x_end) return true;
        x_pos = x_end + 1;
    }
    return false;
}
