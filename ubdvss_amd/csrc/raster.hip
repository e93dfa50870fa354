// Training label maps on device: object quads -> 1/scale-resolution polygon fill.
//
// Reference: SegmapManager.build_segmentation_map (semantic_segmentation/segmap_manager.py:81-104) divides every quad by
// `scale`, snaps the corners outward (_proper_round, :106-133) and fills the polygon with PIL's ImageDraw.polygon, later
// objects over earlier ones, value = class id + 1 (or 1).  The fill rule is Pillow's (libImaging/Draw.c polygon_generic;
// third-party, not in the reference tree), restated from its published behaviour and pinned against the installed Pillow by
// fuzzing (oracle/label_raster.py, tests/test_oracle_raster.py): per scanline the x intersections of the non-horizontal
// edges in float32 (x0 + (y - y0) * dx, product and sum rounded separately), an edge's lower end point counted twice, spans
// [round-half-up(left), round-half-down(right)], horizontal edges drawn as they are, and the single pixel of a top / bottom
// corner -- any two edges leaning to the same side that start (last row: end) in one point -- joined to the span of the
// neighbouring row.  Bit-identical to Pillow 12.2 on convex, concave and self-intersecting quadrilaterals alike (0 differences
// on 50 000 arbitrary quads); the one exception, a quad whose opposite corners coincide (four edges in one point), is drawn with the same rule and logged by the host mirror
// (about 4 % of random such quads then differ from Pillow inside one row; strict_markup refuses them).
// Markup is float64 (rescaled / augmented quads are fractional): the division by the scale and _proper_round's comparisons
// and floor / ceil run in double precision exactly as numpy / math do in the reference.
//
// One thread per map pixel; objects are tested in order and the last one that covers the pixel wins (painter's order).
#include "common.h"
#include "raster_fill.h"       // rq_covers: the scan-line rule, shared with visualize.hip
#include "raster_round.h"      // rq_proper_round: the corner snapping, shared with score.hip

__global__ __launch_bounds__(256) void build_label_maps_kernel(const double *__restrict__ quads, const int *__restrict__ values,
                                                               const int *__restrict__ counts, int n, int cap, int map_h,
                                                               int map_w, int scale, int *__restrict__ labels)
{
    const long total = (long)n * map_h * map_w;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int img = (int)(p / ((long)map_h * map_w));
        const int loc = (int)(p - (long)img * map_h * map_w);
        const int py = loc / map_w, px = loc - py * map_w;
        int cnt = counts[img];
        cnt = cnt < cap ? cnt : cap;
        int label = 0;
        for (int o = 0; o < cnt; ++o) {
            int pts[8];
            rq_proper_round(quads + ((size_t)img * cap + o) * 8, scale, pts);
            if (rq_covers(pts, px, py, map_h)) label = values[(size_t)img * cap + o];
        }
        labels[p] = label;
    }
}

extern "C" int ubd_build_label_maps(const double *quads, const int32_t *values, const int32_t *counts, int n, int cap,
                                    int map_h, int map_w, int scale, int32_t *labels, void *stream)
{
    UBD_REQUIRE(quads && values && counts && labels, "ubd_build_label_maps: null argument");
    UBD_REQUIRE(n > 0 && cap > 0 && map_h > 0 && map_w > 0 && scale > 0, "ubd_build_label_maps: bad shape");
    const long total = (long)n * map_h * map_w;
    int grid = (int)((total + 255) / 256);
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(build_label_maps_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, quads, values, counts, n, cap, map_h, map_w, scale, labels);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ polygon markup (ubd_build_label_maps_polygons)
// Markup read from segmentation maps (markup_readers.py:257-285) is a convex hull of up to UBD_POLY_MAX_VERTS vertices, not a
// quad.  The reference does not snap such a polygon: it divides by the scale and truncates (segmap_manager.py:114-116), then
// fills it with the same ImageDraw.polygon.  polygon_fill.h states the fill rule for n edges.
//
// One block per (image, map row).  The block walks the objects in order and paints into an LDS copy of the row, so painter's
// order needs no ordering between blocks; the row is stored once at the end.  A quad goes through rq_proper_round and rq_covers,
// one lane per pixel: the pixels ubd_build_label_maps writes for it.  Lane t paints the pixels x = t (mod 256) in every path.  Any other polygon: the lanes of wave 0 each take an edge
// and write its intersections with the row into LDS (positions from a ballot prefix count, the edge order of the sequential
// rule), wave 0 rank-sorts the short list, then every lane walks the sorted pairs and paints its pixels of the spans.
#include "polygon_fill.h"
#define PL_THREADS 256
#define PL_MAX_W 8192                   // ints of the LDS row
static_assert(PF_MAX_VERTS == UBD_POLY_MAX_VERTS && PF_MAX_VERTS <= 64, "one edge per lane of a wave");

__global__ __launch_bounds__(PL_THREADS) void build_label_maps_polygons_kernel(const double *__restrict__ verts, const int *__restrict__ nverts,
                                                                               const int *__restrict__ values, const int *__restrict__ counts,
                                                                               int cap, int max_verts, int map_h, int map_w, int scale,
                                                                               int *__restrict__ labels)
{
    extern __shared__ int s_row[];                                  // map_w ints
    __shared__ int s_vx[PF_MAX_VERTS], s_vy[PF_MAX_VERTS];
    __shared__ float s_xx[PF_MAX_X], s_xs[PF_MAX_X];
    __shared__ int s_nx;
    const int py = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    for (int x = tid; x < map_w; x += PL_THREADS) s_row[x] = 0;
    int cnt = counts[img];
    cnt = cnt < cap ? cnt : cap;
    for (int o = 0; o < cnt; ++o) {
        const int nv = nverts[(size_t)img * cap + o];
        const int value = values[(size_t)img * cap + o];
        const double *v = verts + ((size_t)img * cap + o) * (size_t)max_verts * 2;
        if (nv < 3 || nv > max_verts) continue;                     // the host rejects these
        if (nv == 4) {
            int pts[8];
            rq_proper_round(v, scale, pts);
            const int y0 = min(min(pts[1], pts[3]), min(pts[5], pts[7])), y1 = max(max(pts[1], pts[3]), max(pts[5], pts[7]));
            if (py < y0 || py > y1) continue;                       // rq_covers is false outside the corners' rows (block-uniform)
            __syncthreads();
            for (int x = tid; x < map_w; x += PL_THREADS)
                if (rq_covers(pts, x, py, map_h)) s_row[x] = value;
            continue;
        }
        __syncthreads();                                            // the previous object is done with the lists
        if (tid < nv) { s_vx[tid] = pf_truncate(v[2 * tid], scale); s_vy[tid] = pf_truncate(v[2 * tid + 1], scale); }
        __syncthreads();
        int ymin, ymax;
        pf_row_range(s_vy, nv, map_h, &ymin, &ymax);
        const bool scan = py >= ymin && py <= ymax;
        if (tid < 64) {                                             // wave 0: one edge per lane
            int entries = 0;
            float x = 0.f, joined = 0.f;
            if (scan && tid < nv) {
                entries = pf_edge_entries(pf_edge_make(s_vx, s_vy, nv, tid), py, ymax);
                if (entries) x = pf_edge_x(s_vx, s_vy, nv, tid, py, ymax, &joined);
            }
            const unsigned long long any = __ballot(entries > 0), two = __ballot(entries == 2);
            const unsigned long long below = (1ull << tid) - 1ull;
            const int pos = __popcll(any & below) + __popcll(two & below);
            if (entries == 2) s_xx[pos] = x;
            if (entries) s_xx[pos + entries - 1] = joined;
            const int nx = __popcll(any) + __popcll(two);
            if (tid == 0) s_nx = nx;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int i = tid; i < nx; i += 64) s_xs[pf_rank(s_xx, nx, i)] = s_xx[i];
        }
        __syncthreads();
        for (int i = 0; i < nv; ++i) {                              // horizontal edges are drawn as they are
            const int j = i + 1 == nv ? 0 : i + 1;
            if (s_vy[i] != py || s_vy[j] != py) continue;
            const int lo = max(min(s_vx[i], s_vx[j]), 0), hi = min(max(s_vx[i], s_vx[j]), map_w - 1);
            for (int x = lo + ((tid - lo) & (PL_THREADS - 1)); x <= hi; x += PL_THREADS) s_row[x] = value;
        }
        if (scan) {
            const int nx = s_nx;
            int i = 1, x_pos = nx ? (int)s_xs[0] : 0, xs, xe;
            while (pf_next_span(s_xs, nx, &i, &x_pos, &xs, &xe)) {
                xs = max(xs, 0); xe = min(xe, map_w - 1);
                for (int x = xs + ((tid - xs) & (PL_THREADS - 1)); x <= xe; x += PL_THREADS) s_row[x] = value;
            }
        }
    }
    __syncthreads();
    int *out = labels + ((size_t)img * map_h + py) * map_w;
    for (int x = tid; x < map_w; x += PL_THREADS) out[x] = s_row[x];
}

extern "C" int ubd_build_label_maps_polygons(const double *verts, const int32_t *nverts, const int32_t *values, const int32_t *counts,
                                             int n, int cap, int max_verts, int map_h, int map_w, int scale, int32_t *labels,
                                             void *stream)
{
    UBD_REQUIRE(verts && nverts && values && counts && labels, "ubd_build_label_maps_polygons: null argument");
    UBD_REQUIRE(n > 0 && cap > 0 && map_h > 0 && map_w > 0 && scale > 0, "ubd_build_label_maps_polygons: bad shape");
    UBD_REQUIRE(max_verts >= 3 && max_verts <= UBD_POLY_MAX_VERTS, "ubd_build_label_maps_polygons: max_verts must be 3..%d, got %d",
                UBD_POLY_MAX_VERTS, max_verts);
    UBD_REQUIRE(map_w <= PL_MAX_W && map_h <= 65535 && n <= 65535, "ubd_build_label_maps_polygons: map_w <= %d, map_h and n <= 65535", PL_MAX_W);
    hipLaunchKernelGGL(build_label_maps_polygons_kernel, dim3(map_h, n), dim3(PL_THREADS), (size_t)map_w * sizeof(int), (hipStream_t)stream,
                       verts, nverts, values, counts, cap, max_verts, map_h, map_w, scale, labels);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
