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

// segmap_manager.py:96 + :106-133 on float64 markup: bbox / scale (IEEE double division, what numpy does for the reference),
// then floor a coordinate when at least two of the four coordinates on the same axis are strictly larger, else ceil
__device__ void rq_proper_round(const double *bbox, int scale, int *out)
{
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = __ddiv_rn(bbox[k], (double)scale);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int larger = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) larger += v[2 * j + (k & 1)] > v[k] ? 1 : 0;
        out[k] = (int)(larger > 1 ? floor(v[k]) : ceil(v[k]));
    }
}

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
