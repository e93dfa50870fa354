// Pillow's bilinear filter for 8-bit images (libImaging/Geometry.c: bilinear_filter8 / bilinear_filter32RGB behind
// ImagingGenericTransform), restated from its published behaviour: the ONE definition of the sampler, shared by the generic
// transform of warp.hip and the object patches of extract.hip.  A source position (sx, sy), in double, taken from the
// transform of the caller:
//   sx < 0 || sx >= w || sy < 0 || sy >= h: the pixel is 0 in every channel (a NaN position, which Pillow leaves undefined,
//     counts as outside here);
//   otherwise sx -= 0.5, sy -= 0.5, x = floor(sx), y = floor(sy), dx = sx - x, dy = sy - y; columns x and x + 1 clamped to
//     [0, w - 1], row y clamped to [0, h - 1]; v1 = p00 + (p01 - p00) dx (the difference is an integer); on row y + 1, if
//     0 <= y + 1 < h, v2 = p10 + (p11 - p10) dx, else v2 = v1; the result v1 + (v2 - v1) dy is truncated to uint8.
// Every unit that includes this is compiled with -ffp-contract=off (build.sh): no product above may be fused into the
// following sum.
// The source is a signed strided view: pixel (x, y) at s + x * xp + y * yp bytes, w x h pixels of C channels; it is read with
// byte loads through the caches.  w == 0 or h == 0 is an empty view: every position is outside it and nothing is read.
#pragma once
#include <stdint.h>

template <int C>
__device__ __forceinline__ void ubd_bilinear_sample(const uint8_t *__restrict__ s, int32_t xp, int32_t yp, int32_t w, int32_t h,
                                                    double sx, double sy, uint8_t *out)
{
    if (!(sx >= 0.0 && sx < w && sy >= 0.0 && sy < h)) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = 0;
        return;
    }
    sx -= 0.5;
    sy -= 0.5;
    const int xi = sx < 0.0 ? (int)floor(sx) : (int)sx;
    const int yi = sy < 0.0 ? (int)floor(sy) : (int)sy;
    const double dx = sx - xi, dy = sy - yi;
    const int x0 = xi < 0 ? 0 : (xi < w ? xi : w - 1);
    const int x1 = xi + 1 < 0 ? 0 : (xi + 1 < w ? xi + 1 : w - 1);
    const int yc = yi < 0 ? 0 : (yi < h ? yi : h - 1);
    const bool second = yi + 1 >= 0 && yi + 1 < h;
    const uint8_t *r0 = s + (int64_t)yc * yp;
    const uint8_t *r1 = s + (int64_t)(second ? yi + 1 : yc) * yp;        // never dereferenced outside the view
    const int64_t o0 = (int64_t)x0 * xp, o1 = (int64_t)x1 * xp;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const int p00 = r0[o0 + ch], p01 = r0[o1 + ch];
        double v1 = p00 + (p01 - p00) * dx, v2 = v1;
        if (second) {
            const int p10 = r1[o0 + ch], p11 = r1[o1 + ch];
            v2 = p10 + (p11 - p10) * dx;
        }
        v1 = v1 + (v2 - v1) * dy;
        out[ch] = (uint8_t)(int)v1;
    }
}
