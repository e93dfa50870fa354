// Mask-blended augmentation stages on the device: the reference's SimplexNoiseAlpha(EdgeDetect / DirectedEdgeDetect) and
// FrequencyNoiseAlpha(first = Multiply, second = ContrastNormalization) (semantic_segmentation/augmentation.py:301-304, :319-323).
// Both have one shape: two differently processed copies of the image (branches `first` and `second`: identity, a 3 x 3
// correlation, or a per-channel affine map) are blended per pixel by a smooth random mask.  The mask is up to three tiny noise
// grids (at most 16 x 16, made on the host where the draws happen), upscaled to the image (nearest / linear / cubic),
// aggregated (max / average) and pushed through a curve (a sigmoid table, or the identity).  include/ubd.h DEFINES the
// computation in integer arithmetic, tests/noise_alpha_oracle.py restates it in numpy, and this kernel matches it bit for bit.
// Parity with imgaug / cv2 is unpinned, as in photometric.hip.
//
// One kernel, noise_alpha_kernel, in the tile and thread shape of photo_tile_kernel: a block of 256 threads owns a 64 x 16
// output tile of one image, a thread makes 4 consecutive pixels of one row (thread t: row t / 16, columns 4 (t % 16) ..), reads
// the image once and writes it once, as dwords where the addresses allow.  Descriptors travel in the kernel arguments in a
// compact form (na_image, 152 bytes): NA_MAX_IMGS = 24 images per launch (24 x 152 + three pointers + the count = 3680 bytes
// of the 4 KB), the block finds its image by the first-block table.
//
// The upscale is separable and exact, so a block does it in two steps instead of 16 taps per pixel and grid:
//   step 0  threads 0..79 make, per grid, the tap entry of each of the tile's 64 columns and 16 rows: the four clamped grid
//           indices and the phase k (na_axis; two integer divisions each), one dword.  The x taps depend only on x, the y taps
//           only on y: they are made once per block, not per pixel.  The grids and the curve go to LDS as they are (uint16).
//   step 1  thread (row ly, grid column gx) sums its grid column over the row's y taps: V[ly][gx] = sum_j Wy_j g[iy_j][gx].
//   step 2  a pixel sums four V of its row over its x taps, sum_i Wx_i V[ly][ix_i], rounds once, aggregates over the grids,
//           looks the curve up, makes both branches and blends.
// NEAREST and LINEAR run through the same four taps with weights (0, 1, 0, 0) and (0, 32 - k, k, 0).
// Exactness: V and the double sum are carried in fp64.  Every value is an integer: the |W| of an axis sum to at most 180224 = 1.375 x 2^17
// (Keys at a = -3/4, phase 16), g <= 2^15, so |V| <= 1.375 x 2^32 and |sum| <= 1.9 x 2^49 < 2^51; with the rounding constant
// 2^33 everything stays below 2^53, where fp64 holds every integer, products and sums are exact in any order (contraction to
// fma changes nothing), the scaling by 2^-34 is exact and floor() is the arithmetic shift.  fp64 fma runs at the full vector
// rate here, a 64-bit integer multiply-add at a quarter of it.  LINEAR: sum <= 1024 x 32768 = 2^25.  Everything after the
// rounding is int32: aggregation <= 3 x 32768; curve (16384 x 128 + 64) < 2^22; FILTER3 and AFFINE as in photometric.hip
// (< 4.9e8 resp. < 2^26); blend 16384 x 255 + 8192 < 2^23.
//
// LDS (13.3 KB for RGB, 10.5 KB for L, so LDS never limits the blocks per CU before the 2048 threads do):
//   tile    (16 + 2) rows of the source tile with a halo of 1, pitch 57 dwords (RGB; 19 for L), reflect-101 resolved while
//           filling, dword loads at a byte phase for interior tiles -- photo_tile_kernel's layout and fill; filled only when a
//           branch is FILTER3, otherwise the thread reads its 4 pixels straight from global memory
//   colsum  V as fp64 [grid 3][row 16][grid column 16], 6 KB
//   taps    [grid 3][64 column entries, 16 row entries] dwords
//   tab     the grids [3][256] and the curve [257], uint16
// Banks: the byte tile as in photometric.hip (16 lanes of a row at a stride of 3 (1) dwords, the odd pitch spreads the two rows of
// a 32-lane half: at worst 2-way).  colsum is read with ds_read_b64 (bank = dword mod 64): a row is 32 dwords, the two rows of a
// 32-lane half take the two halves of the bank row, and the 16 lanes of a row read at most a few distinct grid columns (4 pixels
// span w / gw-th of a cell; equal addresses broadcast), so the reads are conflict-free unless the grid is finer than the image.
// A lane's four x entries are one aligned 16-byte read; the curve reads are data dependent (two neighbouring uint16 per pixel).
// Bound: the image moves once in each direction like FILTER3; per pixel and grid the kernel adds 4 fp64 fma + the weights
// (about 30 vector instructions), so with three cubic grids it is bound by the vector ALU, not by memory or LDS (DESIGN.md has the figures).
#include "photo_shared.h"

#define NA_MAX_IMGS 24          // images per launch: 152 bytes of descriptor each in the kernel arguments (limit 4 KB)
#define NA_MAX_ITER 3
#define NA_MAX_GRID 16
#define NA_ROWS (PH_TH + 2)
#define NA_TAPS (PH_TW + PH_TH) // tap entries per grid: the tile's columns, then its rows
#define NA_CURVE 257
static_assert(PH_TW / PH_PX == NA_MAX_GRID && PH_THREADS == PH_TH * NA_MAX_GRID, "step 1 maps thread t to (row t / 16, grid column t % 16)");

struct na_image {
    int64_t src_off, dst_off;
    int64_t grid_off[NA_MAX_ITER], curve_off;   // uint16 units into the tables
    int32_t w, h;
    int32_t block0, tiles_x;                    // block0: first block of this image in the launch
    int32_t kinds;                              // first | second << 4 | aggregation << 8 | iterations << 12
    int32_t grid[NA_MAX_ITER];                  // gw | gh << 8 | upscale << 16
    int32_t p[2][9];                            // the branches' parameters
};

struct na_launch {
    na_image img[NA_MAX_IMGS];
    int32_t m;
};
static_assert(sizeof(na_launch) + 3 * sizeof(void *) <= 4096, "the descriptors travel in the kernel arguments");

// The tap entry of coordinate x on an axis of n pixels over gn grid cells: the four clamped grid indices (4 bits each; taps
// i - 1 .. i + 2, replicate border) and the phase k << 16.  NEAREST: all four indices are the cell, k = 0.  cv2.resize's
// pixel-centre rule: X = (2 x + 1) gn - n >= gn - n > -2 n, so a negative X floors to i = -1; X < 2^20.  x may lie past the
// image (the tile's overhang): the indices stay clamped and k in 0..31, the value is never stored.
__device__ __forceinline__ uint32_t na_axis(int x, int n, int gn, int up)
{
    if (up == UBD_NA_NEAREST) return (uint32_t)min(gn - 1, (x * gn) / n) * 0x1111u;
    const int X = (2 * x + 1) * gn - n;
    const int i = X < 0 ? -1 : X / (2 * n);
    const int r = X - i * 2 * n;                                        // 0 .. 2 n - 1
    const int k = (16 * r) / n;                                         // = 32 r / 2 n, 0..31
    uint32_t e = (uint32_t)k << 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) e |= (uint32_t)min(max(i - 1 + j, 0), gn - 1) << (4 * j);
    return e;
}

__device__ __forceinline__ void na_weights(int up, int k, int wgt[4])
{
    if (up == UBD_NA_CUBIC) {
        ph_keys(k, wgt);
    } else {
        wgt[0] = wgt[3] = 0;
        wgt[1] = up == UBD_NA_LINEAR ? 32 - k : 1;
        wgt[2] = up == UBD_NA_LINEAR ? k : 0;
    }
}

// One branch for the thread's 4 pixels: in = the pixels themselves; r[dy] (FILTER3 only) = the LDS byte of the tile row above /
// of / below the pixels' row at the column left of the first pixel
template <int C>
__device__ __forceinline__ void na_branch(int kind, const int32_t *p, const uint8_t *in, const uint8_t *const r[3], uint8_t *out)
{
    if (kind == UBD_NA_FILTER3) {
        int acc[PH_PX * C];
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) acc[k] = 8192;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int k = 0; k < PH_PX; ++k)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) acc[k * C + ch] += p[dy * 3 + dx] * (int)r[dy][(k + dx) * C + ch];
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) out[k] = (uint8_t)ph_shift_clamp<14>(acc[k]);
    } else if (kind == UBD_NA_AFFINE) {
#pragma unroll
        for (int k = 0; k < PH_PX; ++k)
#pragma unroll
            for (int ch = 0; ch < C; ++ch) out[k * C + ch] = (uint8_t)ph_shift_clamp<16>(p[ch] * (int)in[k * C + ch] + p[3 + ch] + 32768);
    } else {
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) out[k] = in[k];
    }
}

template <int C>
__global__ __launch_bounds__(PH_THREADS) void noise_alpha_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                                 const uint16_t *__restrict__ tables, na_launch L)
{
    typedef ph_tile_shape<C> S;
    __shared__ __attribute__((aligned(16))) uint8_t tile[NA_ROWS * S::IN_PITCH];
    __shared__ double colsum[NA_MAX_ITER * PH_TH * NA_MAX_GRID];
    __shared__ __attribute__((aligned(16))) uint32_t taps[NA_MAX_ITER * NA_TAPS];
    __shared__ uint16_t tab[NA_MAX_ITER * 256 + NA_CURVE + 1];
    int b = 0;
    for (int i = 1; i < L.m; ++i)
        if ((int)blockIdx.x >= L.img[i].block0) b = i;                   // block0 is non-decreasing
    const na_image &d = L.img[b];
    const int t = (int)blockIdx.x - d.block0;
    const int ty0 = (t / d.tiles_x) * PH_TH, tx0 = (t - (t / d.tiles_x) * d.tiles_x) * PH_TW;
    const int w = d.w, h = d.h, tid = threadIdx.x;
    const int kind_f = d.kinds & 15, kind_s = (d.kinds >> 4) & 15, aggregation = (d.kinds >> 8) & 15, iters = (d.kinds >> 12) & 15;
    const bool f3 = kind_f == UBD_NA_FILTER3 || kind_s == UBD_NA_FILTER3;
    const uint8_t *s = src + d.src_off;

    // ---- step 0: the grids and the curve, the tap entries of the tile's columns and rows
    for (int it = 0; it < iters; ++it) {
        const int gw = d.grid[it] & 255, gh = (d.grid[it] >> 8) & 255, up = d.grid[it] >> 16;
        if (tid < gw * gh) tab[it * 256 + tid] = tables[d.grid_off[it] + tid];               // gw gh <= 256
        if (tid < PH_TW) taps[it * NA_TAPS + tid] = na_axis(tx0 + tid, w, gw, up);
        else if (tid < NA_TAPS) taps[it * NA_TAPS + tid] = na_axis(ty0 + tid - PH_TW, h, gh, up);
    }
    for (int i = tid; i < NA_CURVE; i += PH_THREADS) tab[NA_MAX_ITER * 256 + i] = tables[d.curve_off + i];

    // ---- the source tile + a halo of 1, reflect-101 resolved here (photo_tile_kernel's fill with hl = hr = 1)
    const int rows = NA_ROWS, cols = PH_TW + 2;
    bool interior = false;
    const int base_phase = (int)((uintptr_t)s & 3);
    const int corner = ((ty0 - 1) * w + (tx0 - 1)) * C;                 // byte offset of the first halo pixel (interior tiles: >= 0)
    if (f3) {
        const int64_t img_bytes = (int64_t)w * h * C;
        interior = tx0 - 1 >= 0 && tx0 + PH_TW + 1 <= w && ty0 - 1 >= 0 && ty0 + PH_TH + 1 <= h;
        if (interior) {
            // the dwords around the first and the last row must stay inside the image's bytes
            const int64_t first = (int64_t)corner - ((base_phase + corner) & 3);
            const int64_t last_end = (int64_t)corner + (int64_t)(rows - 1) * w * C + cols * C;
            const int64_t last_up = last_end + ((4 - ((base_phase + last_end) & 3)) & 3);
            interior = first >= 0 && last_up <= img_bytes;
        }
        if (interior) {
            for (int i = tid; i < rows * S::IN_DWORDS; i += PH_THREADS) {
                const int ly = i / S::IN_DWORDS, k = i - ly * S::IN_DWORDS;
                const int off = corner + ly * w * C;                    // < 2^31: inside the image
                const int phase = (base_phase + off) & 3;
                if (4 * k < phase + cols * C)
                    *(uint32_t *)(tile + ly * S::IN_PITCH + 4 * k) = *(const uint32_t *)(s + (off - phase) + 4 * k);
            }
        } else {
            for (int i = tid; i < rows * cols; i += PH_THREADS) {
                const int ly = i / cols, lx = i - ly * cols;
                const int sy = ph_reflect(ty0 - 1 + ly, h), sx = ph_reflect(tx0 - 1 + lx, w);
                const uint8_t *p = s + ((int64_t)sy * w + sx) * C;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) tile[ly * S::IN_PITCH + lx * C + ch] = p[ch];
            }
        }
    }
    __syncthreads();

    // ---- step 1: V[ly][gx] = sum_j Wy_j g[iy_j][gx], exact in fp64
    const int ly = tid / NA_MAX_GRID, gx = tid - ly * NA_MAX_GRID;
    for (int it = 0; it < iters; ++it) {
        const int gw = d.grid[it] & 255, up = d.grid[it] >> 16;
        if (gx < gw) {
            const uint32_t e = taps[it * NA_TAPS + PH_TW + ly];
            int wy[4];
            na_weights(up, (int)(e >> 16), wy);
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v += (double)wy[j] * (double)tab[it * 256 + (int)((e >> (4 * j)) & 15) * gw + gx];
            colsum[(it * PH_TH + ly) * NA_MAX_GRID + gx] = v;
        }
    }
    __syncthreads();

    // ---- step 2: 4 pixels of one row per thread
    const int x4 = gx * PH_PX, y = ty0 + ly, x = tx0 + x4;
    if (y >= h || x >= w) return;
    const int cnt = w - x < PH_PX ? w - x : PH_PX;
    int agg[PH_PX];
#pragma unroll
    for (int k = 0; k < PH_PX; ++k) agg[k] = 0;
    for (int it = 0; it < iters; ++it) {
        const int up = d.grid[it] >> 16;
        // the one rounding of the upscale: NEAREST the value itself, LINEAR (sum + 512) >> 10, CUBIC (sum + 2^33) >> 34
        const double half = up == UBD_NA_CUBIC ? 8589934592.0 : (up == UBD_NA_LINEAR ? 512.0 : 0.0);
        const double inv = up == UBD_NA_CUBIC ? 5.8207660913467407e-11 : (up == UBD_NA_LINEAR ? 0.0009765625 : 1.0);     // 2^-34, 2^-10
        const double *v = colsum + (it * PH_TH + ly) * NA_MAX_GRID;
        const uint4 e4 = *(const uint4 *)(taps + it * NA_TAPS + x4);
        const uint32_t e[PH_PX] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int k = 0; k < PH_PX; ++k) {
            int wx[4];
            na_weights(up, (int)(e[k] >> 16), wx);
            double sum = half;
#pragma unroll
            for (int i = 0; i < 4; ++i) sum += (double)wx[i] * v[(e[k] >> (4 * i)) & 15];
            const int u = (int)fmin(fmax(floor(sum * inv), 0.0), 32768.0);
            agg[k] = aggregation == UBD_NA_MAX ? max(agg[k], u) : agg[k] + u;
        }
    }
    int alpha[PH_PX];
    const uint16_t *curve = tab + NA_MAX_ITER * 256;
#pragma unroll
    for (int k = 0; k < PH_PX; ++k) {
        int u = agg[k];
        if (aggregation == UBD_NA_AVG) u = iters == 3 ? (u + 1) / 3 : (u + (iters >> 1)) >> (iters - 1);
        const int i = u >> 7, f = u & 127;                              // i = 256 only with f = 0: T[min(i + 1, 256)] then has weight 0
        alpha[k] = ((int)curve[i] * (128 - f) + (int)curve[min(i + 1, NA_CURVE - 1)] * f + 64) >> 7;
    }

    union { uint8_t bytes[PH_PX * C]; uint32_t words[C]; } in, fo, so, o;
    const uint8_t *r[3] = {tile, tile, tile};
    if (f3) {
        // LDS row l starts at tile + l IN_PITCH + (its phase); r[dy] = the byte of row ly + dy at LDS column x4 (image column x - 1)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
            r[dy] = tile + (ly + dy) * S::IN_PITCH + (interior ? ((base_phase + corner + (ly + dy) * w * C) & 3) : 0) + x4 * C;
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) in.bytes[k] = r[1][C + k];
    } else {
        const uint8_t *p = s + ((int64_t)y * w + x) * C;
        if (cnt == PH_PX && (((uintptr_t)p) & 3) == 0) {
#pragma unroll
            for (int k = 0; k < C; ++k) in.words[k] = ((const uint32_t *)p)[k];
        } else {
#pragma unroll
            for (int k = 0; k < PH_PX * C; ++k) in.bytes[k] = k < cnt * C ? p[k] : 0;
        }
    }
    na_branch<C>(kind_f, d.p[0], in.bytes, r, fo.bytes);
    na_branch<C>(kind_s, d.p[1], in.bytes, r, so.bytes);
#pragma unroll
    for (int k = 0; k < PH_PX; ++k)
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
            o.bytes[k * C + ch] = (uint8_t)((alpha[k] * (int)fo.bytes[k * C + ch] + (16384 - alpha[k]) * (int)so.bytes[k * C + ch] + 8192) >> 14);
    uint8_t *q = dst + d.dst_off + ((int64_t)y * w + x) * C;
    if (cnt == PH_PX && (((uintptr_t)q) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < C; ++k) ((uint32_t *)q)[k] = o.words[k];
    } else {
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k)
            if (k < cnt * C) q[k] = o.bytes[k];
    }
}

static int na_check_branch(const ubd_noise_alpha_branch &br, const char *name, int i)
{
    UBD_REQUIRE(br.kind >= UBD_NA_IDENTITY && br.kind <= UBD_NA_AFFINE,
                "ubd_noise_alpha_images: image %d: branch %s has kind %d (0 identity, 1 filter3, 2 affine)", i, name, br.kind);
    if (br.kind == UBD_NA_FILTER3)
        for (int k = 0; k < 9; ++k)
            UBD_REQUIRE(br.p[k] >= -PH_MAX_TAP && br.p[k] <= PH_MAX_TAP, "ubd_noise_alpha_images: image %d: branch %s: tap %d is %d, |tap| must be <= %d",
                        i, name, k, br.p[k], PH_MAX_TAP);
    if (br.kind == UBD_NA_AFFINE)
        for (int k = 0; k < 3; ++k)
            UBD_REQUIRE(br.p[k] >= -(1 << 17) && br.p[k] <= (1 << 17) && br.p[3 + k] >= -(1 << 24) && br.p[3 + k] <= (1 << 24),
                        "ubd_noise_alpha_images: image %d: branch %s: channel %d: m = %d, a = %d, |m| must be <= 2^17 and |a| <= 2^24", i, name, k,
                        br.p[k], br.p[3 + k]);
    return 0;
}

extern "C" int ubd_noise_alpha_images(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, const ubd_noise_alpha_desc *descs,
                                      const uint16_t *tables, size_t table_count, int channels, int n, void *stream)
{
    UBD_REQUIRE(src && dst && descs && tables, "ubd_noise_alpha_images: null argument");
    UBD_REQUIRE(n >= 1, "ubd_noise_alpha_images: n must be >= 1, got %d", n);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_noise_alpha_images: channels must be 1 or 3, got %d", channels);
    for (int i = 0; i < n; ++i) {
        const ubd_noise_alpha_desc &d = descs[i];
        UBD_REQUIRE(d.w >= 1 && d.w <= PH_MAX_SIDE && d.h >= 1 && d.h <= PH_MAX_SIDE,
                    "ubd_noise_alpha_images: image %d is %d x %d, sides must be 1..%d", i, d.h, d.w, PH_MAX_SIDE);
        const int64_t bytes = (int64_t)d.w * d.h * channels;
        static_assert((int64_t)PH_MAX_SIDE * PH_MAX_SIDE * 3 < ((int64_t)1 << 31), "an image of the largest sides stays below 2^31 bytes");
        UBD_REQUIRE(d.src_offset >= 0 && (uint64_t)d.src_offset <= src_bytes && (uint64_t)bytes <= src_bytes - (uint64_t)d.src_offset,
                    "ubd_noise_alpha_images: image %d: source spans bytes [%lld, %lld) of a buffer of %zu", i, (long long)d.src_offset,
                    (long long)(d.src_offset + bytes), src_bytes);
        UBD_REQUIRE(d.dst_offset >= 0 && (uint64_t)d.dst_offset <= dst_bytes && (uint64_t)bytes <= dst_bytes - (uint64_t)d.dst_offset,
                    "ubd_noise_alpha_images: image %d: destination spans bytes [%lld, %lld) of a buffer of %zu", i, (long long)d.dst_offset,
                    (long long)(d.dst_offset + bytes), dst_bytes);
        const uintptr_t sa = (uintptr_t)src + (uintptr_t)d.src_offset, da = (uintptr_t)dst + (uintptr_t)d.dst_offset;
        UBD_REQUIRE(!(sa < da + (uintptr_t)bytes && da < sa + (uintptr_t)bytes),
                    "ubd_noise_alpha_images: image %d: the branches read neighbours, source and destination must not overlap", i);
        if (int rc = na_check_branch(d.first, "first", i)) return rc;
        if (int rc = na_check_branch(d.second, "second", i)) return rc;
        UBD_REQUIRE(d.iterations >= 1 && d.iterations <= NA_MAX_ITER, "ubd_noise_alpha_images: image %d: %d iterations, must be 1..%d", i, d.iterations,
                    NA_MAX_ITER);
        UBD_REQUIRE(d.aggregation == UBD_NA_MAX || d.aggregation == UBD_NA_AVG, "ubd_noise_alpha_images: image %d: aggregation %d (0 max, 1 avg)", i,
                    d.aggregation);
        for (int k = 0; k < d.iterations; ++k) {
            const ubd_noise_alpha_grid &g = d.grid[k];
            UBD_REQUIRE(g.gw >= 1 && g.gw <= NA_MAX_GRID && g.gh >= 1 && g.gh <= NA_MAX_GRID,
                        "ubd_noise_alpha_images: image %d: grid %d is %d x %d, sides must be 1..%d", i, k, g.gh, g.gw, NA_MAX_GRID);
            UBD_REQUIRE(g.upscale >= UBD_NA_NEAREST && g.upscale <= UBD_NA_CUBIC,
                        "ubd_noise_alpha_images: image %d: grid %d: upscale %d (0 nearest, 1 linear, 2 cubic)", i, k, g.upscale);
            UBD_REQUIRE(g.grid_offset >= 0 && (uint64_t)g.grid_offset <= table_count && (uint64_t)(g.gw * g.gh) <= table_count - (uint64_t)g.grid_offset,
                        "ubd_noise_alpha_images: image %d: grid %d spans values [%lld, %lld) of %zu tables values", i, k, (long long)g.grid_offset,
                        (long long)(g.grid_offset + g.gw * g.gh), table_count);
        }
        UBD_REQUIRE(d.curve_offset >= 0 && (uint64_t)d.curve_offset <= table_count && (uint64_t)NA_CURVE <= table_count - (uint64_t)d.curve_offset,
                    "ubd_noise_alpha_images: image %d: the curve spans values [%lld, %lld) of %zu tables values", i, (long long)d.curve_offset,
                    (long long)(d.curve_offset + NA_CURVE), table_count);
    }
    const int64_t lim = (int64_t)1 << 31;
    for (int i = 0; i < n;) {
        na_launch L{};
        int64_t blocks = 0;
        int m = 0;
        for (; i < n && m < NA_MAX_IMGS; ++i) {
            const ubd_noise_alpha_desc &d = descs[i];
            na_image &g = L.img[m++];
            g.src_off = d.src_offset; g.dst_off = d.dst_offset; g.curve_off = d.curve_offset;
            g.w = d.w; g.h = d.h;
            g.kinds = d.first.kind | d.second.kind << 4 | d.aggregation << 8 | d.iterations << 12;
            for (int k = 0; k < d.iterations; ++k) {
                g.grid_off[k] = d.grid[k].grid_offset;
                g.grid[k] = d.grid[k].gw | d.grid[k].gh << 8 | d.grid[k].upscale << 16;
            }
            for (int k = 0; k < 9; ++k) { g.p[0][k] = d.first.p[k]; g.p[1][k] = d.second.p[k]; }
            g.block0 = (int)blocks;
            g.tiles_x = (d.w + PH_TW - 1) / PH_TW;
            blocks += (int64_t)g.tiles_x * ((d.h + PH_TH - 1) / PH_TH);
        }
        L.m = m;
        UBD_REQUIRE(blocks < lim, "ubd_noise_alpha_images: internal: %lld blocks in one launch", (long long)blocks);
        if (channels == 3)
            hipLaunchKernelGGL(noise_alpha_kernel<3>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, tables, L);
        else
            hipLaunchKernelGGL(noise_alpha_kernel<1>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, tables, L);
        UBD_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
