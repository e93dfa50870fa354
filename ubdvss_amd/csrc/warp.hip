// Geometric augmentation on the device: batched, ragged 8-bit warps (rotation, perspective) plus exact index maps (crops,
// quarter turns), the image half of the reference's SegLinksImageAugmentation (semantic_segmentation/augmentation.py:50-85,
// :165-216), which calls Pillow's Image.rotate(angle, BILINEAR, expand=True), Image.crop, and
// Image.transform(size, PERSPECTIVE, coeffs, BILINEAR) on the host at full source resolution.
//
// This file restates Pillow's generic transform with the bilinear filter (libImaging/Geometry.c: ImagingGenericTransform,
// affine_transform, perspective_transform, bilinear_filter8 / bilinear_filter32RGB; third-party, not in the reference tree)
// from its published behaviour, pinned against the installed Pillow by tests/test_gpu_warp.py:
//   per output pixel (x, y): xin = x + 0.5, yin = y + 0.5;
//     affine:      sx = a0 xin + a1 yin + a2,  sy = a3 xin + a4 yin + a5;
//     perspective: the same two numerators, each divided by a6 xin + a7 yin + 1;       all in double, in this order;
//   sx < 0 || sx >= w || sy < 0 || sy >= h: the pixel is 0 in every channel (a NaN position, which Pillow leaves undefined,
//     counts as outside here);
//   otherwise sx -= 0.5, sy -= 0.5, x = floor(sx), y = floor(sy), dx = sx - x, dy = sy - y; columns x and x + 1 clamped to
//     [0, w - 1], row y clamped to [0, h - 1]; v1 = p00 + (p01 - p00) dx (the difference is an integer); on row y + 1, if
//     0 <= y + 1 < h, v2 = p10 + (p11 - p10) dx, else v2 = v1; the result v1 + (v2 - v1) dy is truncated to uint8.
// build.sh compiles this file with -ffp-contract=off: no product above may be fused into the following sum.
// The second half (from the outside test on) is ubd_bilinear_sample of bilinear_sample.h, which extract.hip samples with too.
//
// Crops and quarter turns: EVERY mode reads its source through a signed strided view (byte offset of the view's pixel
// (0, 0), signed byte pitch per view column and per view row, view width and height).  A crop moves the offset and shrinks
// the view, Image.transpose(ROTATE_90 / 180 / 270) permutes and negates the pitches, and both compose on the host without a
// pass of their own: they only feed the next resampling pass, or -- when the chain ends with them -- one pass of the third
// mode, UBD_WARP_COPY, which writes the view out as a packed image.
//
// Lanes: the destination image is one packed byte range, so a lane takes FOUR consecutive pixels of the flat pixel index
// (they may straddle a row end) and, where the image's first byte sits on a dword boundary, stores them as 1 (L) or 3 (RGB)
// aligned dwords; the tail of an image and images at odd addresses take byte stores.  Neighbouring lanes therefore read
// neighbouring source pixels for the angles and coefficients the chain draws; the source is read with byte loads through
// the view (any address, any pitch sign), the caches join the lanes' overlapping neighbourhoods.  One block = 1024
// consecutive pixels of one image; the grid is the concatenation of the images' blocks (descriptors in the kernel
// arguments, at most WP_MAX_IMGS per launch, the block finds its image by the first-block table).
#include "common.h"
#include "bilinear_sample.h"
#include <algorithm>
#include <cmath>

#define WP_MAX_IMGS 32          // images per launch: 112 bytes of descriptor each in the kernel arguments (limit 4 KB)
#define WP_MAX_SIDE 16384
#define WP_THREADS 256
#define WP_PX 4                 // pixels per lane

struct wp_image {
    double a[8];
    int64_t src_off, dst_off;   // bytes from src / dst
    int32_t xp, yp;             // signed source pitches in bytes (per view column, per view row)
    int32_t sw, sh, dw, dh;
    int32_t mode, block0;       // block0: first block of this image in the launch
};

struct wp_launch {
    wp_image img[WP_MAX_IMGS];
    int32_t m;
};

template <int C>
__device__ __forceinline__ void wp_pixel(const uint8_t *__restrict__ s, const wp_image &d, int x, int y, uint8_t *out)
{
    if (d.mode == UBD_WARP_COPY) {
        const uint8_t *p = s + (int64_t)y * d.yp + (int64_t)x * d.xp;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = p[ch];
        return;
    }
    const double xin = x + 0.5, yin = y + 0.5;
    double sx = d.a[0] * xin + d.a[1] * yin + d.a[2];
    double sy = d.a[3] * xin + d.a[4] * yin + d.a[5];
    if (d.mode == UBD_WARP_PERSPECTIVE) {
        const double q = d.a[6] * xin + d.a[7] * yin + 1;
        sx = sx / q;
        sy = sy / q;
    }
    ubd_bilinear_sample<C>(s, d.xp, d.yp, d.sw, d.sh, sx, sy, out);      // the outside test and the filter: bilinear_sample.h
}

template <int C>
__global__ __launch_bounds__(WP_THREADS) void warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, wp_launch L)
{
    int b = 0;
    for (int i = 1; i < L.m; ++i)
        if ((int)blockIdx.x >= L.img[i].block0) b = i;                   // block0 is non-decreasing
    const wp_image &d = L.img[b];
    const int npx = d.dw * d.dh;                                        // < 2^31 (checked on the host)
    const int64_t p0 = ((int64_t)((int)blockIdx.x - d.block0) * WP_THREADS + threadIdx.x) * WP_PX;
    if (p0 >= npx) return;
    const uint8_t *s = src + d.src_off;
    uint8_t *q = dst + d.dst_off + p0 * C;
    int y = (int)(p0 / d.dw), x = (int)(p0 - (int64_t)y * d.dw);
    const int cnt = npx - p0 < WP_PX ? (int)(npx - p0) : WP_PX;
    union { uint8_t bytes[WP_PX * C]; uint32_t words[C]; } o;
#pragma unroll
    for (int k = 0; k < WP_PX; ++k) {
        if (k < cnt) wp_pixel<C>(s, d, x, y, o.bytes + k * C);
        if (++x == d.dw) { x = 0; ++y; }
    }
    if (cnt == WP_PX && (((uintptr_t)(dst + d.dst_off)) & 3) == 0) {     // p0 * C is a multiple of 4
#pragma unroll
        for (int k = 0; k < C; ++k) ((uint32_t *)q)[k] = o.words[k];
    } else {
#pragma unroll
        for (int k = 0; k < WP_PX * C; ++k)
            if (k < cnt * C) q[k] = o.bytes[k];
    }
}

extern "C" int ubd_warp_images(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, const ubd_warp_desc *descs,
                               int channels, int n, void *stream)
{
    UBD_REQUIRE(src && dst && descs, "ubd_warp_images: null argument");
    UBD_REQUIRE(n >= 1, "ubd_warp_images: n must be >= 1, got %d", n);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_warp_images: channels must be 1 or 3, got %d", channels);
    const int64_t lim = (int64_t)1 << 31;
    for (int i = 0; i < n; ++i) {
        const ubd_warp_desc &d = descs[i];
        UBD_REQUIRE(d.mode == UBD_WARP_COPY || d.mode == UBD_WARP_AFFINE || d.mode == UBD_WARP_PERSPECTIVE,
                    "ubd_warp_images: image %d has mode %d (0 copy, 1 affine, 2 perspective)", i, d.mode);
        UBD_REQUIRE(d.src_w >= 1 && d.src_w <= WP_MAX_SIDE && d.src_h >= 1 && d.src_h <= WP_MAX_SIDE && d.dst_w >= 1 &&
                    d.dst_w <= WP_MAX_SIDE && d.dst_h >= 1 && d.dst_h <= WP_MAX_SIDE,
                    "ubd_warp_images: image %d is %d x %d -> %d x %d, sides must be 1..%d", i, d.src_h, d.src_w, d.dst_h, d.dst_w, WP_MAX_SIDE);
        UBD_REQUIRE((int64_t)d.src_w * d.src_h * channels < lim && (int64_t)d.dst_w * d.dst_h * channels < lim,
                    "ubd_warp_images: image %d has 2^31 bytes or more (%d x %d -> %d x %d, %d channels)", i, d.src_h, d.src_w, d.dst_h,
                    d.dst_w, channels);
        UBD_REQUIRE(d.mode != UBD_WARP_COPY || (d.src_w == d.dst_w && d.src_h == d.dst_h),
                    "ubd_warp_images: image %d: copy mode needs equal sizes, got %d x %d -> %d x %d", i, d.src_h, d.src_w, d.dst_h, d.dst_w);
        // the four corners of the source view and the packed destination stay inside the two buffers
        const int64_t ex = (int64_t)(d.src_w - 1) * d.src_xpitch, ey = (int64_t)(d.src_h - 1) * d.src_ypitch;
        const int64_t lo = d.src_offset + std::min<int64_t>(ex, 0) + std::min<int64_t>(ey, 0);
        const int64_t hi = d.src_offset + std::max<int64_t>(ex, 0) + std::max<int64_t>(ey, 0) + channels;
        UBD_REQUIRE(lo >= 0 && hi >= 0 && (uint64_t)hi <= src_bytes,
                    "ubd_warp_images: image %d: source view spans bytes [%lld, %lld) of a buffer of %zu", i, (long long)lo, (long long)hi, src_bytes);
        const int64_t dend = d.dst_offset + (int64_t)d.dst_w * d.dst_h * channels;
        UBD_REQUIRE(d.dst_offset >= 0 && (uint64_t)dend <= dst_bytes,
                    "ubd_warp_images: image %d: destination spans bytes [%lld, %lld) of a buffer of %zu", i, (long long)d.dst_offset,
                    (long long)dend, dst_bytes);
        const int nc = d.mode == UBD_WARP_COPY ? 0 : (d.mode == UBD_WARP_AFFINE ? 6 : 8);
        for (int k = 0; k < nc; ++k)
            UBD_REQUIRE(std::isfinite(d.coeffs[k]), "ubd_warp_images: image %d: coefficient %d is not finite", i, k);
    }
    for (int i0 = 0; i0 < n; i0 += WP_MAX_IMGS) {
        const int m = std::min(WP_MAX_IMGS, n - i0);
        wp_launch L{};
        L.m = m;
        int64_t blocks = 0;
        for (int k = 0; k < m; ++k) {
            const ubd_warp_desc &d = descs[i0 + k];
            wp_image &g = L.img[k];
            for (int c = 0; c < 8; ++c) g.a[c] = d.coeffs[c];
            g.src_off = d.src_offset; g.dst_off = d.dst_offset;
            g.xp = d.src_xpitch; g.yp = d.src_ypitch;
            g.sw = d.src_w; g.sh = d.src_h; g.dw = d.dst_w; g.dh = d.dst_h;
            g.mode = d.mode; g.block0 = (int)blocks;
            blocks += ((int64_t)d.dst_w * d.dst_h + WP_THREADS * WP_PX - 1) / (WP_THREADS * WP_PX);
        }
        UBD_REQUIRE(blocks < lim, "ubd_warp_images: internal: %lld blocks in one launch", (long long)blocks);
        if (channels == 3)
            hipLaunchKernelGGL(warp_kernel<3>, dim3((unsigned)blocks), dim3(WP_THREADS), 0, (hipStream_t)stream, src, dst, L);
        else
            hipLaunchKernelGGL(warp_kernel<1>, dim3((unsigned)blocks), dim3(WP_THREADS), 0, (hipStream_t)stream, src, dst, L);
        UBD_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
