// Pillow's ImageDraw.polygon fill rule for integer polygons of any vertex count, one scan line at a time: the rule of
// raster_fill.h (float32 intersections with product and sum rounded separately, an edge's lower end point counted twice, the
// corner-joining pass in polygon order, horizontal edges drawn as they are, spans [round-half-up(left), round-half-down(right)],
// the running x_pos) for n edges instead of four.  oracle/label_raster.py fill_polygon is the sequential statement of it.
//
// The scan line is cut into steps that are each the work of ONE edge (or one list entry), so that raster.hip can give the edges
// to the lanes of a wave and keep the list in LDS, while the host loops over them:
//   pf_edge_make      edge i of the polygon
//   pf_edge_entries   how many intersections edge i adds to the row (0, 1, or 2 at its lower end point)
//   pf_edge_x         the intersection, corner-joined against the active edges before it in polygon order
//   pf_rank           where an entry of the unsorted list goes in the sorted one
//   pf_next_span      the walk over the sorted pairs with the running x_pos
// pf_row_spans strings them together sequentially; tests/test_polygon_fill_host.py builds it for the host (-ffp-contract=off,
// the rounding intrinsics defined away) and requires Pillow's pixels from it.  raster.hip strings the same steps together
// across a wave.  Every unit that includes this is built with -ffp-contract=off.
#pragma once

#define PF_MAX_VERTS 64                  // = UBD_POLY_MAX_VERTS
#define PF_MAX_X (2 * PF_MAX_VERTS)      // intersections of one row

struct pf_edge { int x0, y0, x1, y1, ymin, ymax; float dx; bool horiz; };

__device__ __forceinline__ int pf_round_up(float f) { return f >= 0.f ? (int)floorf(__fadd_rn(f, 0.5f)) : -(int)floorf(__fadd_rn(fabsf(f), 0.5f)); }
__device__ __forceinline__ int pf_round_down(float f) { return f >= 0.f ? (int)ceilf(__fsub_rn(f, 0.5f)) : -(int)ceilf(__fsub_rn(fabsf(f), 0.5f)); }
__device__ __forceinline__ float pf_x_at(const pf_edge &e, int y) { return __fadd_rn(__fmul_rn((float)(y - e.y0), e.dx), (float)e.x0); }

// segmap_manager.py:114-116: a polygon that is not a quad is divided by the scale (IEEE double, as numpy does) and truncated
__device__ __forceinline__ int pf_truncate(double v, int scale) { return (int)__ddiv_rn(v, (double)scale); }

__device__ __forceinline__ pf_edge pf_edge_make(const int *vx, const int *vy, int n, int i)
{
    const int j = i + 1 == n ? 0 : i + 1;
    pf_edge e;
    e.x0 = vx[i]; e.y0 = vy[i]; e.x1 = vx[j]; e.y1 = vy[j];
    e.ymin = e.y0 < e.y1 ? e.y0 : e.y1; e.ymax = e.y0 < e.y1 ? e.y1 : e.y0;
    e.horiz = e.y0 == e.y1;
    e.dx = e.horiz ? 0.f : __fdiv_rn((float)(e.x1 - e.x0), (float)(e.y1 - e.y0));
    return e;
}

// rows the scan runs over: Pillow starts from ymin = h - 1, ymax = 0, widens them by every edge, then clips to [0, h]
__device__ __forceinline__ void pf_row_range(const int *vy, int n, int map_h, int *ymin, int *ymax)
{
    int lo = map_h - 1, hi = 0;
    for (int i = 0; i < n; ++i) { lo = vy[i] < lo ? vy[i] : lo; hi = vy[i] > hi ? vy[i] : hi; }
    *ymin = lo > 0 ? lo : 0; *ymax = hi < map_h ? hi : map_h;
}

__device__ __forceinline__ bool pf_edge_active(const pf_edge &e, int py) { return !e.horiz && py >= e.ymin && py <= e.ymax; }

// an edge's lower end point counts twice, except in the last row
__device__ __forceinline__ int pf_edge_entries(const pf_edge &e, int py, int ymax)
{
    if (!pf_edge_active(e, py)) return 0;
    return (py == e.ymax && py < ymax) ? 2 : 1;
}

// Intersection of active edge i with row py, after "connect discontiguous corners": two edges leaning to the same side that both
// start in one point of this row (in the last row: both end there) -- the later edge's LAST entry moves towards the span of the
// neighbouring row.  Edges before i in polygon order, first match only.  *joined is that last entry; the return value is the
// plain intersection (the first of two entries keeps it).
__device__ __forceinline__ float pf_edge_x(const int *vx, const int *vy, int n, int i, int py, int ymax, float *joined)
{
    const pf_edge b = pf_edge_make(vx, vy, n, i);
    const float x = pf_x_at(b, py);
    *joined = x;
    if (b.dx == 0.f) return x;
    const int bex = b.y0 == py ? b.x0 : b.x1, bey = b.y0 == py ? b.y0 : b.y1;
    for (int k = 0; k < i; ++k) {
        const pf_edge a = pf_edge_make(vx, vy, n, k);
        if (!pf_edge_active(a, py)) continue;
        if ((b.dx > 0.f && a.dx <= 0.f) || (b.dx < 0.f && a.dx >= 0.f)) continue;
        const bool top = a.ymin == py && b.ymin == py && py < ymax;
        const bool bottom = a.ymax == py && b.ymax == py && py == ymax;
        if (top == bottom) continue;
        const int aex = a.y0 == py ? a.x0 : a.x1, aey = a.y0 == py ? a.y0 : a.y1;
        if (aex != bex || aey != bey) continue;
        const float v = (float)aex;
        const int ya = top ? py + 1 : py - 1;
        const float xa = pf_x_at(a, ya), xb = pf_x_at(b, ya);
        const float lo = fminf(xa, xb), hi = fmaxf(xa, xb);
        if (lo > v) *joined = fmaxf(v, (float)(pf_round_up(lo) - 1));
        else if (hi < v) *joined = fminf(v, __fadd_rn(hi, 1.f));
        break;
    }
    return x;
}

// position of xx[i] in the sorted list (ties by index)
__device__ __forceinline__ int pf_rank(const float *xx, int nx, int i)
{
    const float v = xx[i];
    int r = 0;
    for (int k = 0; k < nx; ++k) r += (xx[k] < v || (xx[k] == v && k < i)) ? 1 : 0;
    return r;
}

// Walk over the sorted intersections: *i starts at 1 and *x_pos at (int)xs[0] (0 for an empty list).  Returns false at the
// end of the list, else true with the next span [*x_start, *x_end], which is empty (start > end) when Pillow skips the pair.
__device__ __forceinline__ bool pf_next_span(const float *xs, int nx, int *i, int *x_pos, int *x_start, int *x_end)
{
    if (*i >= nx) return false;
    const int k = *i;
    *i = k + 2;
    *x_start = 1; *x_end = 0;
    const int e = pf_round_down(xs[k]);
    if (e < *x_pos) return true;
    int s = pf_round_up(xs[k - 1]);
    if (*x_pos > s) { s = *x_pos; if (e < s) return true; }
    if (s > e) return true;
    *x_start = s; *x_end = e; *x_pos = e + 1;
    return true;
}

// The sequential form.  spans: room for 2 * (n + PF_MAX_VERTS) ints, inclusive [start, end] pairs in row py of a canvas of map_h
// rows, unclipped in x; returns how many pairs.  The horizontal edges of the row come first, then the scan line's spans.
__device__ inline int pf_row_spans(const int *vx, const int *vy, int n, int py, int map_h, int *spans)
{
    int ns = 0, ymin, ymax;
    for (int i = 0; i < n; ++i) {
        const pf_edge e = pf_edge_make(vx, vy, n, i);
        if (e.horiz && e.y0 == py) { spans[2 * ns] = e.x0 < e.x1 ? e.x0 : e.x1; spans[2 * ns + 1] = e.x0 < e.x1 ? e.x1 : e.x0; ++ns; }
    }
    pf_row_range(vy, n, map_h, &ymin, &ymax);
    if (py < ymin || py > ymax) return ns;
    float xx[PF_MAX_X], xs[PF_MAX_X];
    int nx = 0;
    for (int i = 0; i < n; ++i) {
        const int cnt = pf_edge_entries(pf_edge_make(vx, vy, n, i), py, ymax);
        if (!cnt) continue;
        float joined;
        const float x = pf_edge_x(vx, vy, n, i, py, ymax, &joined);
        if (cnt == 2) xx[nx++] = x;
        xx[nx++] = joined;
    }
    for (int i = 0; i < nx; ++i) xs[pf_rank(xx, nx, i)] = xx[i];
    int i = 1, x_pos = nx ? (int)xs[0] : 0, s, e;
    while (pf_next_span(xs, nx, &i, &x_pos, &s, &e))
        if (s <= e) { spans[2 * ns] = s; spans[2 * ns + 1] = e; ++ns; }
    return ns;
}
