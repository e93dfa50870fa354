// Rectified patches of the found objects: one upright uint8 patch of a fixed size per object, cut out of the ORIGINAL frames on
// the device from the (quads, counts) that ubd_postprocess left in device memory -- the hand-over to a decoder, which on the host
// is one Image.transform((patch_w, patch_h), Image.QUAD, data, Image.BILINEAR) per object on frames copied back first.
//
// This file restates Pillow's QUAD transform (Image.__transformer's QUAD data, libImaging/Geometry.c: quad_transform; third-party,
// not in the reference tree) from its published behaviour, in front of the bilinear filter of bilinear_sample.h; both pinned against
// the installed Pillow by tests/test_object_patches_host.py through the numpy restatement tests/object_patches_oracle.py, which
// the device matches bit for bit (tests/test_gpu_object_patches.py).  All floating point is double; build.sh compiles this file
// with -ffp-contract=off: no product below may be fused into the following sum.  Per object (image i, slot j < min(counts[i], cap)):
//   1. the corners (x_k, y_k), k = 0..3, are read as int32;
//   2. with scales: X_k = trunc(clamp(x_k * xscale, -2^30, 2^30)), Y_k likewise with yscale (truncation toward zero: the
//      astype(int) of utils.rescale_bbox, what ModelRunner.rescale returns); without: X_k = x_k;
//   3. orientation, in int64: A2 = sum_k (X_k Y_{k+1} - X_{k+1} Y_k) over the cyclic order (y-down: A2 > 0 is clockwise on the
//      screen); A2 < 0 takes the corners in the order 0, 3, 2, 1; with the corners now c_0..c_3, e01 = |c_1 - c_0|^2,
//      e12 = |c_2 - c_1|^2, r = 0 if e01 >= e12 else 1, and NW, NE, SE, SW = c_r, c_{r+1}, c_{r+2}, c_{r+3} (indices mod 4): the
//      patch's width runs along a long side and the patch is a rotation of the object, never a mirror image (the half turn stays
//      open); A2 == 0 counts as clockwise;
//   4. patch_quads[i, j] = NW, NE, SE, SW, the integers of step 3;
//   5. expand != 1: cx = (double)((X_0 + X_1) + (X_2 + X_3)) * 0.25, P_x = cx + ((double)X - cx) * expand per corner, y likewise;
//   6. As = 1.0 / patch_w, At = 1.0 / patch_h; a0 = NW_x, a1 = (NE_x - NW_x) * As, a2 = (SW_x - NW_x) * At,
//      a3 = ((((SE_x - SW_x) - NE_x) + NW_x) * As) * At; a4..a7 the same from y;
//   7. patch pixel (x, y): xin = x + 0.5, yin = y + 0.5, sx = ((a0 + a1 xin) + a2 yin) + (a3 xin) yin, sy likewise from a4..a7;
//   8. ubd_bilinear_sample at (sx, sy) in the image's w x h.
// For a rectangle (what minAreaRect makes) a3 = a7 = 0 up to rounding and the map is affine: the patch is an exact rectification.
// For any other quad it is Pillow's bilinear corner map, not a perspective one.
//
// Lanes: as in warp.hip a lane takes FOUR consecutive pixels of the patch's flat pixel index and one block 1024 of them; the grid
// is flat over (image, slot, block of the patch).  A block whose slot holds no object returns after one load of counts[i].  The
// quad, the scales and the image descriptor sit at block-uniform addresses (scalar loads), every lane forms the eight
// coefficients itself: no LDS, no barrier, no atomics, every output byte written once by one lane.  patch_h * patch_w * channels
// need not be a multiple of 4, so the patches of one call start at every alignment: dword stores where the patch's first byte is
// on a dword boundary and the four pixels are whole, byte stores otherwise.  The descriptors are device memory, so an image that
// does not lie inside src_bytes cannot be refused on the host: the kernel makes it an empty view, which the sampler never reads.
#include "common.h"
#include "bilinear_sample.h"
#include <cmath>

#define EX_THREADS 256
#define EX_PX 4                 // pixels per lane
#define EX_MAX_SIDE 1024

template <int C>
__global__ __launch_bounds__(EX_THREADS) void extract_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
                                                             const int64_t *__restrict__ src_offsets, const int32_t *__restrict__ src_hw,
                                                             const int32_t *__restrict__ quads, const int32_t *__restrict__ counts, int cap,
                                                             const double *__restrict__ scales, double expand, uint8_t *__restrict__ patches,
                                                             int ph, int pw, int bpp, int32_t *__restrict__ patch_quads)
{
    const int slot = (int)blockIdx.x / bpp, blk = (int)blockIdx.x - slot * bpp;   // slot < n * cap < 2^31 (checked on the host)
    const int i = slot / cap, j = slot - i * cap;
    if (j >= counts[i]) return;                                         // j < cap already: slots j >= min(counts[i], cap) hold no object
    const int npx = ph * pw;                                            // <= 2^20
    const int p0 = (blk * EX_THREADS + (int)threadIdx.x) * EX_PX;

    // 1, 2: corners, rescaled
    const int32_t *qp = quads + (int64_t)slot * 8;
    int64_t X[4], Y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { X[k] = qp[2 * k]; Y[k] = qp[2 * k + 1]; }
    if (scales) {
        const double xs = scales[2 * i], ys = scales[2 * i + 1], lim = 1073741824.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double vx = (double)X[k] * xs, vy = (double)Y[k] * ys;
            X[k] = (int64_t)(!(vx >= -lim) ? -lim : (vx > lim ? lim : vx));  // a NaN product goes to the lower bound
            Y[k] = (int64_t)(!(vy >= -lim) ? -lim : (vy > lim ? lim : vy));
        }
    }
    // 3: orientation
    uint64_t area2 = 0;                                                 // summed modulo 2^64: exact for |coordinates| <= 2^30, defined beyond
#pragma unroll
    for (int k = 0; k < 4; ++k) area2 += (uint64_t)X[k] * (uint64_t)Y[(k + 1) & 3] - (uint64_t)X[(k + 1) & 3] * (uint64_t)Y[k];
    if ((int64_t)area2 < 0) {
        int64_t t = X[1]; X[1] = X[3]; X[3] = t;
        t = Y[1]; Y[1] = Y[3]; Y[3] = t;
    }
    const uint64_t d01x = (uint64_t)(X[1] - X[0]), d01y = (uint64_t)(Y[1] - Y[0]), d12x = (uint64_t)(X[2] - X[1]), d12y = (uint64_t)(Y[2] - Y[1]);
    const uint64_t e01 = d01x * d01x + d01y * d01y, e12 = d12x * d12x + d12y * d12y;
    if (e01 < e12) {                                                    // r = 1: rotate the cycle by one
        int64_t t = X[0]; X[0] = X[1]; X[1] = X[2]; X[2] = X[3]; X[3] = t;
        t = Y[0]; Y[0] = Y[1]; Y[1] = Y[2]; Y[2] = Y[3]; Y[3] = t;
    }                                                                   // X, Y = NW, NE, SE, SW
    // 4
    if (patch_quads && blk == 0 && threadIdx.x < 8) {                   // lanes 0..7 of the patch's first block, whatever the patch's size
        int64_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((int)threadIdx.x >> 1 == k) v = (threadIdx.x & 1) ? Y[k] : X[k];
        patch_quads[(int64_t)slot * 8 + threadIdx.x] = (int32_t)v;
    }
    if (p0 >= npx) return;
    // 5: expansion about the centre
    double px[4], py[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { px[k] = (double)X[k]; py[k] = (double)Y[k]; }
    if (expand != 1.0) {
        const double cx = (double)((X[0] + X[1]) + (X[2] + X[3])) * 0.25, cy = (double)((Y[0] + Y[1]) + (Y[2] + Y[3])) * 0.25;
#pragma unroll
        for (int k = 0; k < 4; ++k) { px[k] = cx + (px[k] - cx) * expand; py[k] = cy + (py[k] - cy) * expand; }
    }
    // 6: Pillow's QUAD data
    const double As = 1.0 / pw, At = 1.0 / ph;
    const double a0 = px[0], a1 = (px[1] - px[0]) * As, a2 = (px[3] - px[0]) * At, a3 = ((((px[2] - px[3]) - px[1]) + px[0]) * As) * At;
    const double a4 = py[0], a5 = (py[1] - py[0]) * As, a6 = (py[3] - py[0]) * At, a7 = ((((py[2] - py[3]) - py[1]) + py[0]) * As) * At;

    // the image: an empty view when it does not lie inside src_bytes
    const int64_t off = src_offsets[i];
    int32_t h = src_hw[2 * i], w = src_hw[2 * i + 1];
    const bool inside = h >= 1 && w >= 1 && (int64_t)w * C < ((int64_t)1 << 31) && off >= 0 && (uint64_t)off <= src_bytes &&
                        (uint64_t)h * (uint64_t)w <= (src_bytes - (uint64_t)off) / C;     // the row pitch w * C is an int32
    if (!inside) h = w = 0;
    const uint8_t *s = src + (inside ? off : 0);

    // 7, 8
    uint8_t *pbase = patches + (int64_t)slot * npx * C;
    uint8_t *q = pbase + (int64_t)p0 * C;
    int y = p0 / pw, x = p0 - y * pw;
    const int cnt = npx - p0 < EX_PX ? npx - p0 : EX_PX;
    union { uint8_t bytes[EX_PX * C]; uint32_t words[C]; } o;
#pragma unroll
    for (int k = 0; k < EX_PX; ++k) {
        if (k < cnt) {
            const double xin = x + 0.5, yin = y + 0.5;
            const double sx = ((a0 + a1 * xin) + a2 * yin) + (a3 * xin) * yin;
            const double sy = ((a4 + a5 * xin) + a6 * yin) + (a7 * xin) * yin;
            ubd_bilinear_sample<C>(s, C, w * C, w, h, sx, sy, o.bytes + k * C);
        }
        if (++x == pw) { x = 0; ++y; }
    }
    if (cnt == EX_PX && (((uintptr_t)pbase) & 3) == 0) {                // p0 * C is a multiple of 4
#pragma unroll
        for (int k = 0; k < C; ++k) ((uint32_t *)q)[k] = o.words[k];
    } else {
#pragma unroll
        for (int k = 0; k < EX_PX * C; ++k)
            if (k < cnt * C) q[k] = o.bytes[k];
    }
}

extern "C" int ubd_extract_objects(const uint8_t *src, size_t src_bytes, const int64_t *src_offsets, const int32_t *src_hw, int channels,
                                   const int32_t *quads, const int32_t *counts, int n, int cap, const double *scales, double expand,
                                   uint8_t *patches, int patch_h, int patch_w, int32_t *patch_quads, void *stream)
{
    UBD_REQUIRE(src, "ubd_extract_objects: src is null");
    UBD_REQUIRE(src_offsets, "ubd_extract_objects: src_offsets is null");
    UBD_REQUIRE(src_hw, "ubd_extract_objects: src_hw is null");
    UBD_REQUIRE(quads, "ubd_extract_objects: quads is null");
    UBD_REQUIRE(counts, "ubd_extract_objects: counts is null");
    UBD_REQUIRE(patches, "ubd_extract_objects: patches is null");
    UBD_REQUIRE(n >= 1, "ubd_extract_objects: n must be >= 1, got %d", n);
    UBD_REQUIRE(cap >= 1, "ubd_extract_objects: cap must be >= 1, got %d", cap);
    UBD_REQUIRE(patch_h >= 1 && patch_h <= EX_MAX_SIDE, "ubd_extract_objects: patch_h must be 1..%d, got %d", EX_MAX_SIDE, patch_h);
    UBD_REQUIRE(patch_w >= 1 && patch_w <= EX_MAX_SIDE, "ubd_extract_objects: patch_w must be 1..%d, got %d", EX_MAX_SIDE, patch_w);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_extract_objects: channels must be 1 or 3, got %d", channels);
    UBD_REQUIRE(std::isfinite(expand) && expand > 0.0, "ubd_extract_objects: expand must be finite and > 0, got %g", expand);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t bpp = ((int64_t)patch_h * patch_w + EX_THREADS * EX_PX - 1) / (EX_THREADS * EX_PX);     // <= 1024
    const int64_t slots = (int64_t)n * cap;
    UBD_REQUIRE(slots < lim && slots * bpp < lim,
                "ubd_extract_objects: n * cap * blocks per patch = %d * %d * %lld is not below 2^31", n, cap, (long long)bpp);
    const dim3 grid((unsigned)(slots * bpp)), block(EX_THREADS);
    if (channels == 3)
        hipLaunchKernelGGL(extract_kernel<3>, grid, block, 0, (hipStream_t)stream, src, (uint64_t)src_bytes, src_offsets, src_hw, quads,
                           counts, cap, scales, expand, patches, patch_h, patch_w, (int)bpp, patch_quads);
    else
        hipLaunchKernelGGL(extract_kernel<1>, grid, block, 0, (hipStream_t)stream, src, (uint64_t)src_bytes, src_offsets, src_hw, quads,
                           counts, cap, scales, expand, patches, patch_h, patch_w, (int)bpp, patch_quads);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
