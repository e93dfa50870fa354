// The reference's corner snapping of a quad at 1/scale resolution, as a device function.  Shared by raster.hip (training label
// maps) and score.hip (the region of a found object): one text, so the two paint the same pixels.  Every unit that includes this
// is built with -ffp-contract=off.  Kept apart from raster_fill.h, which tests/test_raster_fill_host.py compiles for the host with
// four float intrinsics defined away: this one needs the double division.
#pragma once

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
