// Photometric augmentation on the device: the built part of the reference's imgaug stage (semantic_segmentation/
// augmentation.py:276-332), one operation per image per call, batched and ragged like warp.hip.  imgaug and OpenCV are third
// party and not available to pin against, so every mode is DEFINED here in integer arithmetic (include/ubd.h lists the
// formulas, each restated from imgaug's published behaviour) and tests/photometric_oracle.py is the same definition in numpy;
// the device must match it bit for bit.  Parity with imgaug / cv2 is unpinned.  The one exception is UBD_PHOTO_NOISE, whose
// Box-Muller transform runs in fp32 with the device's logf / cosf: build.sh compiles this file with -ffp-contract=off so that
// no product is fused into a sum, and the tests excuse only pixels whose exact value lies within 1e-4 (1 + scale) of a rounding
// boundary.
//
// Two kernels, descriptors in the kernel arguments (PH_MAX_IMGS per launch, 88 bytes each), the block finds its image by the
// first-block table, as in warp.hip:
//
// photo_point_kernel (AFFINE, GREY, NOISE, DROPOUT).  The image is one packed byte range; a lane takes four consecutive pixels of
// the flat pixel index (= y w + x, the Philox counter) and moves them as 1 (L) or 3 (RGB) dwords where the image's first source /
// destination byte sits on a dword boundary, as bytes otherwise and at the image's tail.  A lane reads only the bytes it writes,
// so source == destination (in place) is safe.  One block = 1024 pixels.
//
// photo_tile_kernel (FILTER3, SEP, BOX).  One block of 256 threads owns a PH_TW x PH_TH = 64 x 16 output tile of one image and
// loads the tile plus the mode's halo (hl columns / rows before, hr after, both <= 4) into LDS once, reflect-101 resolved while
// filling, so the passes index LDS without bounds tests.  A tile whose halo lies inside the image reads whole dwords of every
// source row (row start rounded down to a dword boundary) and stores them as dwords; the row then sits in LDS at the byte phase
// (row address & 3), which the readers add.  Border tiles and the first / last bytes of an image take byte loads, phase 0.
// Tile shape: 64 pixels = 192 contiguous output bytes per row for RGB, 16 lanes x 12 bytes, stored as dwords where the image is
// dword aligned; 16 rows keep the halo overhead of the widest mode at (72 x 24) / (64 x 16) = 1.7 loads per output byte (the
// re-reads hit L2) with 15 KB of LDS per block, so several blocks share a CU.
// LDS layouts: the byte tile has a row pitch of 57 dwords (RGB; 19 for L): a lane reads bytes at a lane stride of 12 (4) bytes =
// 3 (1) dwords, 16 lanes of a row touch 16 different banks, and the odd pitch (25 mod 32, 19 mod 32) spreads the two rows of a
// 32-lane group, so the byte reads are at worst 2-way.  The 16-bit row-pass results of SEP / BOX (t <= 32640 resp. 1785) have a
// pitch of 97 (33) dwords: a lane's 12 (4) values are 6 (2) dwords, 16 lanes take the even banks, the next row the odd ones.
// Each thread makes 4 consecutive pixels of one row in every pass: the row pass LDS -> LDS over TH + hl + hr rows (BOX as a
// running sum along the row), then the column pass LDS -> registers -> global.
// Ranges (all int32): AFFINE |m v + a + 32768| < 2^17 255 + 2^24 + 2^15 < 2^26; GREY 16384 255 + 8192 < 2^23; FILTER3
// 9 taps |tap| <= 13 16384 times 255: 9 13 16384 255 + 8192 < 4.9e8 < 2^31; SEP rows sum w v <= 16384 255 < 2^23, t <= 32640,
// columns sum w t <= 16384 32640 + 2^20 < 2^30; BOX S <= 49 255, 2 S + k k < 2^15.
#include "common.h"
#include <algorithm>
#include <cmath>

#define PH_MAX_IMGS 32          // images per launch: 88 bytes of descriptor each in the kernel arguments (limit 4 KB)
#define PH_MAX_SIDE 16384
#define PH_THREADS 256
#define PH_PX 4                 // pixels per lane
#define PH_TW 64
#define PH_TH 16
#define PH_HALO 4
#define PH_ROWS (PH_TH + 2 * PH_HALO)
#define PH_MAX_TAP (13 * 16384)

struct ph_image {
    int64_t src_off, dst_off;
    uint64_t seed;
    int32_t w, h, mode, flags;
    int32_t block0, tiles_x;    // block0: first block of this image in the launch
    int32_t p[10];
};

struct ph_launch {
    ph_image img[PH_MAX_IMGS];
    int32_t m;
};

__device__ __forceinline__ int ph_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// clamp(v >> n, 0, 255) as a clamp of v followed by a logical shift of the non-negative value: the same number (the shift is
// monotonic), and two instructions (v_med3_i32, v_lshrrev_b32) whose result needs no masking when the bytes are packed
template <int N> __device__ __forceinline__ int ph_shift_clamp(int v)
{
    const int top = (256 << N) - 1;
    v = v < 0 ? 0 : (v > top ? top : v);
    return (int)((unsigned)v >> N);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"), counter (c0, 0, j, 0)
__device__ __forceinline__ void ph_philox(uint32_t c0, uint32_t j, uint64_t seed, uint32_t r[4])
{
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c1 = 0, c2 = j, c3 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ float ph_normal(uint32_t a, uint32_t b)
{
    const float u1 = ((float)(a >> 9) + 0.5f) * 1.1920928955078125e-7f;     // 2^-23; (a >> 9) + 0.5 is exact in fp32
    const float u2 = ((float)(b >> 9) + 0.5f) * 1.1920928955078125e-7f;
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795864769f * u2);
}

template <int C>
__device__ __forceinline__ void ph_point(const ph_image &d, uint32_t pixel, const uint8_t *in, uint8_t *out)
{
    if (d.mode == UBD_PHOTO_AFFINE) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = (uint8_t)ph_shift_clamp<16>(d.p[ch] * (int)in[ch] + d.p[3 + ch] + 32768);
    } else if (d.mode == UBD_PHOTO_GREY) {
        if (C == 3) {
            const int g = (4899 * in[0] + 9617 * in[1 % C] + 1868 * in[2 % C] + 8192) >> 14, aq = d.p[0];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) out[ch] = (uint8_t)(((16384 - aq) * (int)in[ch] + aq * g + 8192) >> 14);
        } else {
            out[0] = in[0];
        }
    } else if (d.mode == UBD_PHOTO_DROPOUT) {
        uint32_t r[4];
        ph_philox(pixel, 0, d.seed, r);
        const uint32_t thr = (uint32_t)d.p[0];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = r[(d.flags & 1) ? ch : 0] < thr ? 0 : in[ch];
    } else {                                                            // UBD_PHOTO_NOISE
        uint32_t r[8];
        ph_philox(pixel, 0, d.seed, r);
        const float scale = __int_as_float(d.p[0]);
        if (C == 3 && (d.flags & 1)) {
            ph_philox(pixel, 1, d.seed, r + 4);
#pragma unroll
            for (int ch = 0; ch < C; ++ch)
                out[ch] = (uint8_t)ph_clamp((int)rintf((float)in[ch] + scale * ph_normal(r[2 * ch], r[2 * ch + 1])));
        } else {
            const float z = scale * ph_normal(r[0], r[1]);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) out[ch] = (uint8_t)ph_clamp((int)rintf((float)in[ch] + z));
        }
    }
}

// no __restrict__: an image may be processed in place
template <int C>
__global__ __launch_bounds__(PH_THREADS) void photo_point_kernel(const uint8_t *src, uint8_t *dst, ph_launch L)
{
    int b = 0;
    for (int i = 1; i < L.m; ++i)
        if ((int)blockIdx.x >= L.img[i].block0) b = i;                   // block0 is non-decreasing
    const ph_image &d = L.img[b];
    const int npx = d.w * d.h;                                          // < 2^31 (checked on the host)
    const int64_t p0 = ((int64_t)((int)blockIdx.x - d.block0) * PH_THREADS + threadIdx.x) * PH_PX;
    if (p0 >= npx) return;
    const uint8_t *s = src + d.src_off + p0 * C;
    uint8_t *q = dst + d.dst_off + p0 * C;
    const int cnt = npx - p0 < PH_PX ? (int)(npx - p0) : PH_PX;
    union { uint8_t bytes[PH_PX * C]; uint32_t words[C]; } in, o;
    const bool full = cnt == PH_PX;
    if (full && (((uintptr_t)(src + d.src_off)) & 3) == 0) {            // p0 * C is a multiple of 4
#pragma unroll
        for (int k = 0; k < C; ++k) in.words[k] = ((const uint32_t *)s)[k];
    } else {
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) in.bytes[k] = k < cnt * C ? s[k] : 0;
    }
#pragma unroll
    for (int k = 0; k < PH_PX; ++k) ph_point<C>(d, (uint32_t)(p0 + k), in.bytes + k * C, o.bytes + k * C);
    if (full && (((uintptr_t)(dst + d.dst_off)) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < C; ++k) ((uint32_t *)q)[k] = o.words[k];
    } else {
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k)
            if (k < cnt * C) q[k] = o.bytes[k];
    }
}

__device__ __forceinline__ int ph_reflect(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

template <int C> struct ph_tile_shape {
    static constexpr int IN_PITCH = C == 3 ? 57 * 4 : 19 * 4;           // bytes; >= 3 + (PH_TW + 2 PH_HALO) C
    static constexpr int IN_DWORDS = C == 3 ? 56 : 19;                  // dwords that can hold source bytes of one row
    static constexpr int T_PITCH = PH_TW * C + 2;                       // ushorts: 97 / 33 dwords
};

template <int C>
__global__ __launch_bounds__(PH_THREADS) void photo_tile_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, ph_launch L)
{
    typedef ph_tile_shape<C> S;
    __shared__ __attribute__((aligned(16))) uint8_t tile[PH_ROWS * S::IN_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t tsum[PH_ROWS * S::T_PITCH];
    int b = 0;
    for (int i = 1; i < L.m; ++i)
        if ((int)blockIdx.x >= L.img[i].block0) b = i;
    const ph_image &d = L.img[b];
    const int t = (int)blockIdx.x - d.block0;
    const int ty0 = (t / d.tiles_x) * PH_TH, tx0 = (t - (t / d.tiles_x) * d.tiles_x) * PH_TW;
    const int w = d.w, h = d.h, mode = d.mode, tid = threadIdx.x;
    int hl, hr;                                                         // halo before / after, on both axes
    if (mode == UBD_PHOTO_FILTER3) hl = hr = 1;
    else if (mode == UBD_PHOTO_SEP) hl = hr = d.p[0];
    else { hl = d.p[0] >> 1; hr = d.p[0] - 1 - hl; }
    const int rows = PH_TH + hl + hr, cols = PH_TW + hl + hr;
    const uint8_t *s = src + d.src_off;
    const int64_t img_bytes = (int64_t)w * h * C;

    // ---- fill: tile + halo, reflect-101 resolved here
    bool interior = tx0 - hl >= 0 && tx0 + PH_TW + hr <= w && ty0 - hl >= 0 && ty0 + PH_TH + hr <= h;
    const int base_phase = (int)((uintptr_t)s & 3);
    const int corner = ((ty0 - hl) * w + (tx0 - hl)) * C;               // byte offset of the first halo pixel (interior tiles: >= 0)
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
            const int off = corner + ly * w * C;                        // < 2^31: inside the image
            const int phase = (base_phase + off) & 3;
            if (4 * k < phase + cols * C)
                *(uint32_t *)(tile + ly * S::IN_PITCH + 4 * k) = *(const uint32_t *)(s + (off - phase) + 4 * k);
        }
    } else {
        for (int i = tid; i < rows * cols; i += PH_THREADS) {
            const int ly = i / cols, lx = i - ly * cols;
            const int sy = ph_reflect(ty0 - hl + ly, h), sx = ph_reflect(tx0 - hl + lx, w);
            const uint8_t *p = s + ((int64_t)sy * w + sx) * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) tile[ly * S::IN_PITCH + lx * C + ch] = p[ch];
        }
    }
    __syncthreads();
    // LDS row ly starts at tile + ly IN_PITCH + (its phase)
    auto row_ptr = [&](int ly) -> const uint8_t * {
        return tile + ly * S::IN_PITCH + (interior ? ((base_phase + corner + ly * w * C) & 3) : 0);
    };

    // ---- row pass of SEP / BOX: t[ly][x][ch] for every LDS row, 4 pixels per item
    if (mode != UBD_PHOTO_FILTER3) {
        for (int i = tid; i < rows * (PH_TW / PH_PX); i += PH_THREADS) {
            const int ly = i / (PH_TW / PH_PX), x4 = (i - ly * (PH_TW / PH_PX)) * PH_PX;
            const uint8_t *r = row_ptr(ly) + x4 * C;                    // LDS column x4 = image column tx0 + x4 - hl
            uint16_t *o = tsum + ly * S::T_PITCH + x4 * C;
            if (mode == UBD_PHOTO_SEP) {
                const int rad = hl;
#pragma unroll
                for (int k = 0; k < PH_PX; ++k)
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        int acc = d.p[1] * (int)r[(k + rad) * C + ch];
                        for (int j = 1; j <= rad; ++j)
                            acc += d.p[1 + j] * ((int)r[(k + rad - j) * C + ch] + (int)r[(k + rad + j) * C + ch]);
                        o[k * C + ch] = (uint16_t)((acc + 64) >> 7);
                    }
            } else {
                const int kk = hl + hr + 1;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    int acc = 0;
                    for (int j = 0; j < kk; ++j) acc += r[j * C + ch];
                    o[ch] = (uint16_t)acc;
#pragma unroll
                    for (int k = 1; k < PH_PX; ++k) {                   // running sum along the row
                        acc += (int)r[(k + kk - 1) * C + ch] - (int)r[(k - 1) * C + ch];
                        o[k * C + ch] = (uint16_t)acc;
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- column pass (SEP / BOX) or the 3 x 3 correlation, 4 pixels of one row per thread, and the store
    const int ly = tid / (PH_TW / PH_PX), x4 = (tid - ly * (PH_TW / PH_PX)) * PH_PX;
    const int y = ty0 + ly, x = tx0 + x4;
    if (y >= h || x >= w) return;
    union { uint8_t bytes[PH_PX * C]; uint32_t words[C]; } o;
    if (mode == UBD_PHOTO_FILTER3) {
        int acc[PH_PX * C];
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) acc[k] = 8192;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const uint8_t *r = row_ptr(ly + dy) + x4 * C;
#pragma unroll
            for (int k = 0; k < PH_PX; ++k)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) acc[k * C + ch] += d.p[dy * 3 + dx] * (int)r[(k + dx) * C + ch];
        }
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) o.bytes[k] = (uint8_t)ph_shift_clamp<14>(acc[k]);
    } else if (mode == UBD_PHOTO_SEP) {
        const int rad = hl;
        const uint16_t *c = tsum + (ly + rad) * S::T_PITCH + x4 * C;
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) {
            int acc = d.p[1] * (int)c[k] + (1 << 20);
            for (int j = 1; j <= rad; ++j) acc += d.p[1 + j] * ((int)c[k - j * S::T_PITCH] + (int)c[k + j * S::T_PITCH]);
            o.bytes[k] = (uint8_t)ph_shift_clamp<21>(acc);
        }
    } else {
        const int kk = hl + hr + 1, k2 = kk * kk;
        const uint16_t *c = tsum + ly * S::T_PITCH + x4 * C;
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k) {
            int acc = 0;
            for (int j = 0; j < kk; ++j) acc += c[k + j * S::T_PITCH];
            o.bytes[k] = (uint8_t)((2 * acc + k2) / (2 * k2));
        }
    }
    uint8_t *q = dst + d.dst_off + ((int64_t)y * w + x) * C;
    const int cnt = w - x < PH_PX ? w - x : PH_PX;
    if (cnt == PH_PX && (((uintptr_t)q) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < C; ++k) ((uint32_t *)q)[k] = o.words[k];
    } else {
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k)
            if (k < cnt * C) q[k] = o.bytes[k];
    }
}

static inline bool ph_is_point(int mode)
{
    return mode == UBD_PHOTO_AFFINE || mode == UBD_PHOTO_GREY || mode == UBD_PHOTO_NOISE || mode == UBD_PHOTO_DROPOUT;
}

extern "C" int ubd_photometric_images(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, const ubd_photo_desc *descs,
                                      int channels, int n, void *stream)
{
    UBD_REQUIRE(src && dst && descs, "ubd_photometric_images: null argument");
    UBD_REQUIRE(n >= 1, "ubd_photometric_images: n must be >= 1, got %d", n);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_photometric_images: channels must be 1 or 3, got %d", channels);
    const int64_t lim = (int64_t)1 << 31;
    for (int i = 0; i < n; ++i) {
        const ubd_photo_desc &d = descs[i];
        UBD_REQUIRE(d.mode >= UBD_PHOTO_AFFINE && d.mode <= UBD_PHOTO_DROPOUT,
                    "ubd_photometric_images: image %d has mode %d (0 affine, 1 grey, 2 filter3, 3 sep, 4 box, 5 noise, 6 dropout)", i, d.mode);
        UBD_REQUIRE(d.w >= 1 && d.w <= PH_MAX_SIDE && d.h >= 1 && d.h <= PH_MAX_SIDE,
                    "ubd_photometric_images: image %d is %d x %d, sides must be 1..%d", i, d.h, d.w, PH_MAX_SIDE);
        const int64_t bytes = (int64_t)d.w * d.h * channels;
        static_assert((int64_t)PH_MAX_SIDE * PH_MAX_SIDE * 3 < ((int64_t)1 << 31), "an image of the largest sides stays below 2^31 bytes");
        UBD_REQUIRE(d.src_offset >= 0 && (uint64_t)d.src_offset <= src_bytes && (uint64_t)bytes <= src_bytes - (uint64_t)d.src_offset,
                    "ubd_photometric_images: image %d: source spans bytes [%lld, %lld) of a buffer of %zu", i, (long long)d.src_offset,
                    (long long)(d.src_offset + bytes), src_bytes);
        UBD_REQUIRE(d.dst_offset >= 0 && (uint64_t)d.dst_offset <= dst_bytes && (uint64_t)bytes <= dst_bytes - (uint64_t)d.dst_offset,
                    "ubd_photometric_images: image %d: destination spans bytes [%lld, %lld) of a buffer of %zu", i, (long long)d.dst_offset,
                    (long long)(d.dst_offset + bytes), dst_bytes);
        const uintptr_t sa = (uintptr_t)src + (uintptr_t)d.src_offset, da = (uintptr_t)dst + (uintptr_t)d.dst_offset;
        const bool overlap = sa < da + (uintptr_t)bytes && da < sa + (uintptr_t)bytes;
        if (ph_is_point(d.mode))
            UBD_REQUIRE(!overlap || sa == da, "ubd_photometric_images: image %d: source and destination overlap without being the same range", i);
        else
            UBD_REQUIRE(!overlap, "ubd_photometric_images: image %d: mode %d reads neighbours, source and destination must not overlap", i, d.mode);
        if (d.mode == UBD_PHOTO_BOX)
            UBD_REQUIRE(d.p[0] >= 2 && d.p[0] <= 7, "ubd_photometric_images: image %d: box size %d, must be 2..7", i, d.p[0]);
        if (d.mode == UBD_PHOTO_SEP) {
            UBD_REQUIRE(d.p[0] >= 1 && d.p[0] <= PH_HALO, "ubd_photometric_images: image %d: radius %d, must be 1..%d", i, d.p[0], PH_HALO);
            int64_t sum = d.p[1];
            for (int k = 0; k <= d.p[0]; ++k) {
                UBD_REQUIRE(d.p[1 + k] >= 0 && d.p[1 + k] <= 16384, "ubd_photometric_images: image %d: weight %d is %d, must be 0..16384", i, k, d.p[1 + k]);
                if (k) sum += 2 * (int64_t)d.p[1 + k];
            }
            UBD_REQUIRE(sum == 16384, "ubd_photometric_images: image %d: the %d weights sum to %lld, must be 16384", i, 2 * d.p[0] + 1, (long long)sum);
        }
        if (d.mode == UBD_PHOTO_FILTER3)
            for (int k = 0; k < 9; ++k)
                UBD_REQUIRE(d.p[k] >= -PH_MAX_TAP && d.p[k] <= PH_MAX_TAP, "ubd_photometric_images: image %d: tap %d is %d, |tap| must be <= %d", i, k,
                            d.p[k], PH_MAX_TAP);
        if (d.mode == UBD_PHOTO_AFFINE)
            for (int k = 0; k < 3; ++k)
                UBD_REQUIRE(d.p[k] >= -(1 << 17) && d.p[k] <= (1 << 17) && d.p[3 + k] >= -(1 << 24) && d.p[3 + k] <= (1 << 24),
                            "ubd_photometric_images: image %d: channel %d: m = %d, a = %d, |m| must be <= 2^17 and |a| <= 2^24", i, k, d.p[k], d.p[3 + k]);
        if (d.mode == UBD_PHOTO_GREY)
            UBD_REQUIRE(d.p[0] >= 0 && d.p[0] <= 16384, "ubd_photometric_images: image %d: alpha %d, must be 0..16384", i, d.p[0]);
        if (d.mode == UBD_PHOTO_NOISE) {
            float scale;
            memcpy(&scale, &d.p[0], 4);
            UBD_REQUIRE(std::isfinite(scale) && scale >= 0.f, "ubd_photometric_images: image %d: noise scale must be finite and >= 0", i);
        }
    }
    // two passes over the descriptors: the pointwise images, then the neighbourhood images, PH_MAX_IMGS per launch
    for (int pass = 0; pass < 2; ++pass) {
        int i = 0;
        while (i < n) {
            ph_launch L{};
            int64_t blocks = 0;
            int m = 0;
            for (; i < n && m < PH_MAX_IMGS; ++i) {
                const ubd_photo_desc &d = descs[i];
                if (ph_is_point(d.mode) != (pass == 0)) continue;
                ph_image &g = L.img[m++];
                g.src_off = d.src_offset; g.dst_off = d.dst_offset; g.seed = d.seed;
                g.w = d.w; g.h = d.h; g.mode = d.mode; g.flags = d.flags;
                for (int k = 0; k < 10; ++k) g.p[k] = d.p[k];
                g.block0 = (int)blocks;
                g.tiles_x = (d.w + PH_TW - 1) / PH_TW;
                blocks += pass == 0 ? ((int64_t)d.w * d.h + PH_THREADS * PH_PX - 1) / (PH_THREADS * PH_PX)
                                    : (int64_t)g.tiles_x * ((d.h + PH_TH - 1) / PH_TH);
            }
            if (!m) break;
            L.m = m;
            UBD_REQUIRE(blocks < lim, "ubd_photometric_images: internal: %lld blocks in one launch", (long long)blocks);
            if (pass == 0) {
                if (channels == 3)
                    hipLaunchKernelGGL(photo_point_kernel<3>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
                else
                    hipLaunchKernelGGL(photo_point_kernel<1>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
            } else {
                if (channels == 3)
                    hipLaunchKernelGGL(photo_tile_kernel<3>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
                else
                    hipLaunchKernelGGL(photo_tile_kernel<1>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
            }
            UBD_CHECK_HIP(hipGetLastError());
        }
    }
    return 0;
}
