// Raw images of any size -> the net's input size on the device (the resize half).
//
// Reference: SegmapManager._rescale_image_and_markup (semantic_segmentation/segmap_manager.py:135-173) resizes every image
// with PIL's Image.resize((new_w, new_h), Image.BICUBIC), and data_generators.py:177 converts it with Image.convert('L') for
// grey nets.  This file restates Pillow's 8-bit resampler (libImaging/Resample.c; third-party, not in the reference tree) from
// its published behaviour, pinned against the installed Pillow by tests/test_gpu_resize.py:
//   per axis that changes size, horizontal first: scale = in / out, fs = max(scale, 1), support = 2 fs;
//   output i: center = (i + 0.5) scale, xmin = max(int(center - support + 0.5), 0), taps n = min(int(center + support + 0.5), in) - xmin,
//   k[x] = bicubic((x + xmin - center + 0.5) * (1 / fs)) (a = -0.5), k /= sum k (sum != 0), all in double;
//   kk = int(k 2^22 +- 0.5) (truncated toward zero); out = clip((2^21 + sum kk[x] p[xmin + x]) >> 22, 0, 255).
// The first pass is clipped to uint8 before the second reads it.  The first pass is the horizontal one, except for images more
// than 100 times as tall as they are wide that shrink vertically: Pillow 12 runs those vertical first (the switch is exactly at
// in_h > 100 in_w and only for a vertical downscale; tests/test_gpu_resize.py pins both sides of it).  An axis whose size does not change gives the
// taps (0, 2^22, 0, 0) around every pixel, i.e. the identity, so it needs no special case.  RGB -> L is
// (R 19595 + G 38470 + B 7471 + 0x8000) >> 16 (Pillow's convert('L')).  The double expressions keep Pillow's operation order;
// build.sh compiles this file with -ffp-contract=off.
//
// One block = (image, band of BR output rows, chunk of BC output columns); both passes in one launch:
//   1. per output column / row of the tile: center, xmin, tap count and the double sum of the weights (one thread each, summed
//      in tap order like Pillow); then the fixed-point taps into LDS tables -- or, where a table would not fit (downscales by
//      hundreds), recomputed per use from the same numbers;
//   2. the source rows of the band's vertical window, in slabs of SR rows: the column span the chunk needs is staged into LDS
//      with aligned dword loads (a source row starts at any byte), and the horizontal pass writes the uint8 intermediate of
//      the window (rows x BC x src_c) into LDS;
//   3. the vertical pass out of LDS, optional RGB -> L or L -> RGB, stores to the NHWC destination.
// A vertical-first image (at most 163 columns wide, see above) takes the other order: the vertical pass over the chunk's column
// span, read straight from the source, into LDS, then the horizontal pass out of LDS.
// Integer sums are exact in 32 bits whatever their order (Pillow's int accumulator shows the final sums fit), and the
// products kk * p take the 24-bit multiply (|kk| < 2^23, p < 2^8).
#include "common.h"
#include <algorithm>
#include <cmath>

#define RS_MAX_IMGS 64          // images per launch: their offsets and sizes travel in the kernel arguments
#define RS_MAX_SIDE_IN 16384
#define RS_MAX_SIDE_OUT 8192
#define RS_THREADS 256
#define RS_LDS_MAX 163840       // what one workgroup may declare on gfx950
#define RS_TABLE_MAX 16384      // bytes of one fixed-point tap table; larger tables are recomputed per use instead

struct rs_images {
    int64_t off[RS_MAX_IMGS];   // byte offset of image i from src
    int32_t h[RS_MAX_IMGS], w[RS_MAX_IMGS];
};

// per output pixel of one axis (Pillow's precompute_coeffs)
struct rs_out {
    double center, ss, ww;
    int x0, n;
};

struct rs_geom {                // per launch: the tile shape and the LDS layout (bytes), bounds over the launch's images
    int bc, br, sr;             // output columns / rows per tile, source rows per slab
    int kh, kv;                 // tap-table row lengths (0: no table, taps recomputed per use)
    int stage_pitch;            // bytes per staged source row (multiple of 4)
    int off_meta_v, off_tab_h, off_tab_v, off_stage, off_inter;
};

__device__ __forceinline__ double rs_bicubic(double x)
{
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__device__ __forceinline__ int rs_fixed(const rs_out &o, int x)
{
    double k = rs_bicubic(((double)(x + o.x0) - o.center + 0.5) * o.ss);
    if (o.ww != 0.0) k = k / o.ww;
    return k < 0 ? (int)(-0.5 + k * (double)(1 << 22)) : (int)(0.5 + k * (double)(1 << 22));
}

__device__ void rs_setup(rs_out &o, int i, int in, int out)
{
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    o.center = (i + 0.5) * scale;
    o.ss = 1.0 / fs;
    int xmin = (int)(o.center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(o.center + support + 0.5);
    if (xmax > in) xmax = in;
    o.x0 = xmin;
    o.n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < o.n; ++x) ww += rs_bicubic(((double)(x + xmin) - o.center + 0.5) * o.ss);
    o.ww = ww;
}

__device__ __forceinline__ int rs_clip8(int ss)
{
    const int v = ss >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// clipped sums of one output pixel -> dst_c bytes (RGB -> L as Pillow's convert('L'), L -> RGB replicated)
template <int SC>
__device__ __forceinline__ void rs_put_pixel(uint8_t *q, const int *acc, int dst_c)
{
    if (SC == 3) {
        const int r = rs_clip8(acc[0]), gg = rs_clip8(acc[SC > 1 ? 1 : 0]), bl = rs_clip8(acc[SC > 2 ? 2 : 0]);
        if (dst_c == 3) { q[0] = (uint8_t)r; q[1] = (uint8_t)gg; q[2] = (uint8_t)bl; }
        else q[0] = (uint8_t)((r * 19595 + gg * 38470 + bl * 7471 + 0x8000) >> 16);
    } else {
        const uint8_t v = (uint8_t)rs_clip8(acc[0]);
        q[0] = v;
        if (dst_c == 3) { q[1] = v; q[2] = v; }
    }
}

template <int SC>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(const uint8_t *__restrict__ src, rs_images imgs, rs_geom g, int img0,
                                                            uint8_t *__restrict__ dst, int dst_h, int dst_w, int dst_c)
{
    extern __shared__ __align__(16) uint8_t rs_lds[];
    rs_out *meta_h = (rs_out *)rs_lds;
    rs_out *meta_v = (rs_out *)(rs_lds + g.off_meta_v);
    int *tab_h = (int *)(rs_lds + g.off_tab_h);
    int *tab_v = (int *)(rs_lds + g.off_tab_v);
    uint8_t *stage = rs_lds + g.off_stage;
    uint8_t *inter = rs_lds + g.off_inter;

    const int b = blockIdx.z;
    const int in_h = imgs.h[b], in_w = imgs.w[b];
    const int i0 = blockIdx.x * g.bc, j0 = blockIdx.y * g.br;
    const int nc = min(g.bc, dst_w - i0), nr = min(g.br, dst_h - j0);
    const int t = threadIdx.x;

    // 1. taps of this tile's output columns and rows
    if (t < nc) rs_setup(meta_h[t], i0 + t, in_w, dst_w);
    if (t >= 128 && t - 128 < nr) rs_setup(meta_v[t - 128], j0 + t - 128, in_h, dst_h);
    __syncthreads();
    if (g.kh)
        for (int e = t; e < nc * g.kh; e += RS_THREADS) {
            const int i = e / g.kh, x = e - i * g.kh;
            tab_h[e] = x < meta_h[i].n ? rs_fixed(meta_h[i], x) : 0;
        }
    if (g.kv)
        for (int e = t; e < nr * g.kv; e += RS_THREADS) {
            const int j = e / g.kv, y = e - j * g.kv;
            tab_v[e] = y < meta_v[j].n ? rs_fixed(meta_v[j], y) : 0;
        }
    const int xbase = meta_h[0].x0;                                   // xmin is non-decreasing in the output index
    const int xspan = meta_h[nc - 1].x0 + meta_h[nc - 1].n - xbase;  // source columns the chunk reads
    const int ybase = meta_v[0].x0;
    const int yend = meta_v[nr - 1].x0 + meta_v[nr - 1].n;           // source rows [ybase, yend) of the band's window
    const size_t pitch = (size_t)in_w * SC;
    const uint8_t *img = src + imgs.off[b];
    const int row_bytes = nc * SC;

    if (in_h > 100 * in_w && dst_h < in_h && dst_w != in_w) {
        // vertical first (Pillow's order for tall, narrow images): rows of the band over the chunk's column span into LDS
        __syncthreads();                                              // tables written
        for (int e = t; e < nr * xspan; e += RS_THREADS) {
            const int j = e / xspan, x = e - j * xspan;
            const rs_out &o = meta_v[j];
            const uint8_t *p = img + (size_t)o.x0 * pitch + (size_t)(xbase + x) * SC;
            int acc[SC];
#pragma unroll
            for (int ch = 0; ch < SC; ++ch) acc[ch] = 1 << 21;
            for (int y = 0; y < o.n; ++y) {
                const int kk = g.kv ? tab_v[j * g.kv + y] : rs_fixed(o, y);
#pragma unroll
                for (int ch = 0; ch < SC; ++ch) acc[ch] += __mul24(kk, (int)p[(size_t)y * pitch + ch]);
            }
#pragma unroll
            for (int ch = 0; ch < SC; ++ch) inter[e * SC + ch] = (uint8_t)rs_clip8(acc[ch]);
        }
        __syncthreads();
        for (int e = t; e < nr * nc; e += RS_THREADS) {
            const int j = e / nc, i = e - j * nc;
            const rs_out &o = meta_h[i];
            const uint8_t *p = inter + (j * xspan + o.x0 - xbase) * SC;
            int acc[SC];
#pragma unroll
            for (int ch = 0; ch < SC; ++ch) acc[ch] = 1 << 21;
            for (int x = 0; x < o.n; ++x) {
                const int kk = g.kh ? tab_h[i * g.kh + x] : rs_fixed(o, x);
#pragma unroll
                for (int ch = 0; ch < SC; ++ch) acc[ch] += __mul24(kk, (int)p[x * SC + ch]);
            }
            rs_put_pixel<SC>(dst + ((((size_t)(img0 + b) * dst_h + j0 + j) * dst_w) + i0 + i) * dst_c, acc, dst_c);
        }
        return;
    }

    // 2. horizontal pass of the window rows, slab by slab
    for (int r0 = ybase; r0 < yend; r0 += g.sr) {
        const int rows = min(g.sr, yend - r0);
        __syncthreads();                                              // tables written / previous slab consumed
        // stage: per row, the aligned dwords that cover bytes [xbase * SC, (xbase + xspan) * SC) of the row
        const int wpr = g.stage_pitch >> 2;
        for (int e = t; e < rows * wpr; e += RS_THREADS) {
            const int rr = e / wpr, wi = e - rr * wpr;
            const uintptr_t first = (uintptr_t)(img + (size_t)(r0 + rr) * pitch + (size_t)xbase * SC);
            const uintptr_t a0 = first & ~(uintptr_t)3;
            const uintptr_t last = first + (uintptr_t)xspan * SC;       // one past the last byte needed
            const uintptr_t a = a0 + (uintptr_t)wi * 4;
            if (a < last)                                             // every loaded dword holds a needed byte: no page is touched that the row does not touch
                ((uint32_t *)(stage + rr * g.stage_pitch))[wi] = *(const uint32_t *)a;
        }
        __syncthreads();
        for (int e = t; e < rows * nc; e += RS_THREADS) {
            const int rr = e / nc, i = e - rr * nc;
            const rs_out &o = meta_h[i];
            const int mis = (int)((uintptr_t)(img + (size_t)(r0 + rr) * pitch + (size_t)xbase * SC) & 3);
            const uint8_t *p = stage + rr * g.stage_pitch + mis + (o.x0 - xbase) * SC;
            int acc[SC];
#pragma unroll
            for (int ch = 0; ch < SC; ++ch) acc[ch] = 1 << 21;
            for (int x = 0; x < o.n; ++x) {
                const int kk = g.kh ? tab_h[i * g.kh + x] : rs_fixed(o, x);
#pragma unroll
                for (int ch = 0; ch < SC; ++ch) acc[ch] += __mul24(kk, (int)p[x * SC + ch]);
            }
            uint8_t *q = inter + (r0 - ybase + rr) * row_bytes + i * SC;
#pragma unroll
            for (int ch = 0; ch < SC; ++ch) q[ch] = (uint8_t)rs_clip8(acc[ch]);
        }
    }
    __syncthreads();

    // 3. vertical pass out of LDS, channel conversion, NHWC stores (consecutive threads: consecutive output columns)
    for (int e = t; e < nr * nc; e += RS_THREADS) {
        const int j = e / nc, i = e - j * nc;
        const rs_out &o = meta_v[j];
        const uint8_t *p = inter + (o.x0 - ybase) * row_bytes + i * SC;
        int acc[SC];
#pragma unroll
        for (int ch = 0; ch < SC; ++ch) acc[ch] = 1 << 21;
        for (int y = 0; y < o.n; ++y) {
            const int kk = g.kv ? tab_v[j * g.kv + y] : rs_fixed(o, y);
#pragma unroll
            for (int ch = 0; ch < SC; ++ch) acc[ch] += __mul24(kk, (int)p[y * row_bytes + ch]);
        }
        rs_put_pixel<SC>(dst + ((((size_t)(img0 + b) * dst_h + j0 + j) * dst_w) + i0 + i) * dst_c, acc, dst_c);
    }
}

// Host copy of rs_setup's tap bounds (no double sums): bounds of the tile's window for the LDS layout.
static int rs_ksize(int in, int out)
{
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    const int k = 2 * (int)ceil(2.0 * fs) + 1;
    return k < in ? k : in;
}

// source positions (columns or rows) that `tile` consecutive outputs read: (tile - 1) * scale + 1 (two truncations) + taps, at most `in`
static int rs_span(int in, int out, int tile)
{
    const double scale = (double)in / out;
    const long s = (long)floor((tile - 1) * scale) + 2 + rs_ksize(in, out);
    return (int)(s < in ? s : in);
}

static size_t rs_align(size_t v) { return (v + 15) & ~(size_t)15; }

struct rs_plan { rs_geom g; size_t lds; };

static rs_plan rs_plan_for(const int32_t *hw, int n, int src_c, int dst_h, int dst_w, int bc, int br, int sr)
{
    int kh = 0, kv = 0, xs = 0, win = 0;
    size_t inter = 0;
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        kh = std::max(kh, rs_ksize(w, dst_w));
        kv = std::max(kv, rs_ksize(h, dst_h));
        xs = std::max(xs, rs_span(w, dst_w, bc));
        win = std::max(win, rs_span(h, dst_h, br));
        const bool vfirst = h > 100 * w && dst_h < h && dst_w != w;   // as in resize_kernel
        inter = std::max(inter, vfirst ? (size_t)br * rs_span(w, dst_w, bc) * src_c : (size_t)rs_span(h, dst_h, br) * bc * src_c);
    }
    rs_plan p{};
    rs_geom &g = p.g;
    g.bc = bc; g.br = br; g.sr = std::min(sr, win);
    g.kh = (size_t)bc * kh * 4 <= RS_TABLE_MAX ? kh : 0;
    g.kv = (size_t)br * kv * 4 <= RS_TABLE_MAX ? kv : 0;
    g.stage_pitch = (int)(((size_t)xs * src_c + 3 + 3) & ~(size_t)3);    // up to 3 bytes of misalignment in front, rounded up to dwords
    size_t o = rs_align(sizeof(rs_out) * bc);
    g.off_meta_v = (int)o;  o = rs_align(o + sizeof(rs_out) * br);
    g.off_tab_h = (int)o;   o = rs_align(o + (size_t)bc * g.kh * 4);
    g.off_tab_v = (int)o;   o = rs_align(o + (size_t)br * g.kv * 4);
    g.off_stage = (int)o;   o = rs_align(o + (size_t)g.sr * g.stage_pitch);
    g.off_inter = (int)o;   o = rs_align(o + inter);
    p.lds = o;
    return p;
}

extern "C" int ubd_resize_images(const uint8_t *src, const int64_t *src_offsets, const int32_t *src_hw, int src_c, int n,
                                 uint8_t *dst, int dst_h, int dst_w, int dst_c, void *stream)
{
    UBD_REQUIRE(src && src_offsets && src_hw && dst, "ubd_resize_images: null argument");
    UBD_REQUIRE(n >= 1, "ubd_resize_images: n must be >= 1, got %d", n);
    UBD_REQUIRE(src_c == 1 || src_c == 3, "ubd_resize_images: src_c must be 1 or 3, got %d", src_c);
    UBD_REQUIRE(dst_c == 1 || dst_c == 3, "ubd_resize_images: dst_c must be 1 or 3, got %d", dst_c);
    UBD_REQUIRE(dst_h >= 1 && dst_h <= RS_MAX_SIDE_OUT && dst_w >= 1 && dst_w <= RS_MAX_SIDE_OUT,
                "ubd_resize_images: destination %d x %d outside 1..%d", dst_h, dst_w, RS_MAX_SIDE_OUT);
    UBD_REQUIRE((int64_t)n * dst_h * dst_w * dst_c < ((int64_t)1 << 31), "ubd_resize_images: destination of %lld bytes is not below 2^31",
                (long long)n * dst_h * dst_w * dst_c);
    for (int i = 0; i < n; ++i) {
        UBD_REQUIRE(src_hw[2 * i] >= 1 && src_hw[2 * i] <= RS_MAX_SIDE_IN && src_hw[2 * i + 1] >= 1 && src_hw[2 * i + 1] <= RS_MAX_SIDE_IN,
                    "ubd_resize_images: image %d is %d x %d, sides must be 1..%d", i, src_hw[2 * i], src_hw[2 * i + 1], RS_MAX_SIDE_IN);
        UBD_REQUIRE(src_offsets[i] >= 0, "ubd_resize_images: image %d has a negative offset %lld", i, (long long)src_offsets[i]);
    }
    int dev = 0;
    UBD_CHECK_HIP(hipGetDevice(&dev));
    static bool attr_set[64][2];                   // the dynamic-LDS limit above 64 KiB is raised once per device and kernel
    for (int i0 = 0; i0 < n; i0 += RS_MAX_IMGS) {
        const int m = std::min(RS_MAX_IMGS, n - i0);
        // tile: up to 64 columns x 16 rows, 16 source rows per slab; shrunk (slab, then rows, then columns) until LDS holds it
        int bc = std::min(64, dst_w), br = std::min(16, dst_h), sr = 16;
        rs_plan p = rs_plan_for(src_hw + 2 * i0, m, src_c, dst_h, dst_w, bc, br, sr);
        while (p.lds > RS_LDS_MAX && (sr > 1 || br > 1 || bc > 1)) {
            if (sr > 1) sr = (sr + 1) / 2;
            else if (br > 1) br = (br + 1) / 2;
            else bc = (bc + 1) / 2;
            p = rs_plan_for(src_hw + 2 * i0, m, src_c, dst_h, dst_w, bc, br, sr);
        }
        UBD_REQUIRE(p.lds <= RS_LDS_MAX, "ubd_resize_images: internal: no tile fits LDS (%zu bytes)", p.lds);
        rs_images imgs{};
        for (int k = 0; k < m; ++k) {
            imgs.off[k] = src_offsets[i0 + k];
            imgs.h[k] = src_hw[2 * (i0 + k)];
            imgs.w[k] = src_hw[2 * (i0 + k) + 1];
        }
        const dim3 grid((dst_w + p.g.bc - 1) / p.g.bc, (dst_h + p.g.br - 1) / p.g.br, m);
        const void *fn = src_c == 3 ? (const void *)resize_kernel<3> : (const void *)resize_kernel<1>;
        if (p.lds > 65536 && dev >= 0 && dev < 64 && !attr_set[dev][src_c == 3]) {
            UBD_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX));
            attr_set[dev][src_c == 3] = true;
        }
        if (src_c == 3)
            hipLaunchKernelGGL(resize_kernel<3>, grid, dim3(RS_THREADS), p.lds, (hipStream_t)stream, src, imgs, p.g, i0, dst, dst_h, dst_w, dst_c);
        else
            hipLaunchKernelGGL(resize_kernel<1>, grid, dim3(RS_THREADS), p.lds, (hipStream_t)stream, src, imgs, p.g, i0, dst, dst_h, dst_w, dst_c);
        UBD_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
