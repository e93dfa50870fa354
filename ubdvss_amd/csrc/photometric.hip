// Photometric augmentation on the device: the built part of the reference's imgaug stage (semantic_segmentation/
// augmentation.py:276-332), one operation per image per call, batched and ragged like warp.hip.  imgaug and OpenCV are third
// party and not available to pin against, so every mode is DEFINED here in integer arithmetic (include/ubd.h lists the
// formulas, each restated from imgaug's published behaviour) and tests/photometric_oracle.py (modes 0..6) and
// tests/photometric_ext_oracle.py (MEDIAN, HSV, ELASTIC) are the same definition in numpy;
// the device must match it bit for bit.  Parity with imgaug / cv2 is unpinned.  The one exception is UBD_PHOTO_NOISE, whose
// Box-Muller transform runs in fp32 with the device's logf / cosf: build.sh compiles this file with -ffp-contract=off so that
// no product is fused into a sum, and the tests excuse only pixels whose exact value lies within 1e-4 (1 + scale) of a rounding
// boundary.
//
// The two remaining entries of that stage, SimplexNoiseAlpha and FrequencyNoiseAlpha (two processed copies of the image blended
// by a smooth random mask), are ubd_noise_alpha_images in noise_alpha.hip; photo_shared.h holds what the two files share.
//
// Four kernels, descriptors in the kernel arguments (PH_MAX_IMGS per launch, 88 bytes each), the block finds its image by the
// first-block table, as in warp.hip:
//
// photo_point_kernel (AFFINE, GREY, NOISE, DROPOUT, HSV).  The image is one packed byte range; a lane takes four consecutive pixels of
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
//
// photo_median_kernel (MEDIAN).  The same 64 x 16 tile and thread shape; the tile plus a halo of k / 2 <= 5 on every side is filled
// with byte loads, coordinates clamped to the image (replicate border), into one byte tile of (16 + 10) rows with a pitch of 57
// dwords (RGB; 19 for L): 5928 (1976) bytes, so LDS never limits the blocks per CU.  A thread makes the medians of 4 consecutive
// pixels of one row = 12 (4) bytes = 3 (1) dwords, which start on a dword of the tile (4 pixels x C bytes).  Selection: an 8-step
// bitwise search on the value, from the top bit down; a step counts the window bytes below the trial value in the four byte
// lanes of a dword at once (ph_median_select has the identities), so 4 output bytes cost k k packed compares per step instead of
// 4 k k.  Per step and window row a lane reads its ceil((4 + k - 1) C / 4) <= 11 (4) consecutive dwords once (ds_read_b32, banks
// dword mod 32 per 32-lane half) and forms the window columns with v_alignbyte_b32.  Bank behaviour: the 16 lanes of a tile row read
// at a stride of 3 dwords (1 for L), 16 different banks; a 32-lane half holds two rows, 57 = 25 (19) mod 32 apart: for RGB three
// lanes of the second row meet a bank of the first, so a read is at worst 2-way; L is conflict-free.  The kernel is bound by the
// packed compares (VALU), not by LDS: 8 k (3 k x 9 VALU) against 8 k x 11 LDS dwords per thread at k = 11, RGB.
//
// photo_elastic_kernel (ELASTIC).  The same tile and thread shape.  The raw field of the tile plus one ring (66 x 18 pixels, one
// Philox call each: 1.16 per output pixel) goes to LDS as packed int16 pairs (ey << 16 | ex), pitch 67 dwords; the row pass writes
// 64 x 18 packed pairs, pitch 65; both passes walk x fastest, so consecutive lanes take consecutive banks.  9512 bytes of LDS.
// Then every thread smooths along the column, and gathers the 4 x 4 source window of each of its 4 pixels from global memory with
// byte loads (the neighbours' windows overlap: L2 / TCP hits), a tap outside the image skipped; rows in int32, the four row sums
// times the column weights in int64.
// Ranges (all int32): AFFINE |m v + a + 32768| < 2^17 255 + 2^24 + 2^15 < 2^26; GREY 16384 255 + 8192 < 2^23; FILTER3
// 9 taps |tap| <= 13 16384 times 255: 9 13 16384 255 + 8192 < 4.9e8 < 2^31; SEP rows sum w v <= 16384 255 < 2^23, t <= 32640,
// columns sum w t <= 16384 32640 + 2^20 < 2^30; BOX S <= 49 255, 2 S + k k < 2^15; HSV products <= 1 044 582; ELASTIC field sums
// <= 16384 32768 + 8192 < 2^30, |aq s| <= 2^27, a row of the gather |sum W v| <= 255 (131072 + 2 x 14553) < 2^26.
#include "photo_shared.h"       // the tile shape, the clamps, ph_reflect, ph_keys: shared with noise_alpha.hip
#include <algorithm>
#include <cmath>

#define PH_MAX_IMGS 32          // images per launch: 88 bytes of descriptor each in the kernel arguments (limit 4 KB)
#define PH_ROWS (PH_TH + 2 * PH_HALO)
#define PH_MED_HALO 5           // MEDIAN: k <= 11
#define PH_EL_RAW_PITCH 67      // ELASTIC: dwords per LDS row of the raw field (66 used) and of the row-pass result (64 used)
#define PH_EL_ROW_PITCH 65

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

// UBD_PHOTO_HSV: OpenCV's 8-bit RGB -> HSV (H 0..179) with its Q12 reciprocals, the shift, and the sector formula back; every
// operand of a division is non-negative (include/ubd.h has the formulas and the ranges)
__device__ __forceinline__ void ph_hsv(int R, int G, int B, int dh, int ds, uint8_t &oR, uint8_t &oG, uint8_t &oB)
{
    const int V = max(R, max(G, B)), D = V - min(R, min(G, B));
    const int sdiv = V ? (int)((2088960u + (unsigned)V) / (2u * (unsigned)V)) : 0;
    const int hdiv = D ? (int)((245760u + (unsigned)D) / (2u * (unsigned)D)) : 0;
    int S = (D * sdiv + 2048) >> 12;
    const int hn = V == R ? G - B : (V == G ? B - R + 2 * D : R - G + 4 * D);
    int H = (hn * hdiv + 2048) >> 12;
    if (H < 0) H += 180;
    H = (H + dh + 360) % 180;                                           // H + dh >= -255
    S = ph_clamp(S + ds);
    const int i = H / 30, f = H - 30 * i;
    const int P = (30 * V * (255 - S) + 3825) / 7650;
    const int Q = (V * (7650 - S * f) + 3825) / 7650;
    const int T = (V * (7650 - S * (30 - f)) + 3825) / 7650;
    const int r = i == 0 || i == 5 ? V : (i == 1 ? Q : (i == 4 ? T : P));
    const int g = i == 1 || i == 2 ? V : (i == 0 ? T : (i == 3 ? Q : P));
    const int b = i == 3 || i == 4 ? V : (i == 2 ? T : (i == 5 ? Q : P));
    oR = (uint8_t)r; oG = (uint8_t)g; oB = (uint8_t)b;
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
    } else if (d.mode == UBD_PHOTO_HSV) {
        if (C == 3) ph_hsv(in[0], in[1 % C], in[2 % C], d.p[0], d.p[1], out[0], out[1 % C], out[2 % C]);
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

// ---------------------------------------------------------------------------------------------------------------- MEDIAN
template <int C> struct ph_med_shape {
    static constexpr int PITCH = C == 3 ? 57 : 19;                      // dwords; >= ceil((PH_TW + 2 PH_MED_HALO) C / 4) = 56 / 19, odd
};

// The medians of 4 C consecutive output bytes (C dwords) of one row, K x K window.  base: the lane's first LDS dword of the
// window's first row; window column j of output dword m starts 4 m + j C bytes further: a compile-time dword index and byte
// shift (v_alignbyte_b32 of two neighbouring dwords).  Eight steps from the top bit down; a step counts, in each of the four
// byte lanes of a dword at once, the window bytes below the trial value: with H = 0x80 in every byte, t = (x | H) - (y & ~H)
// has bit 7 set where the low 7 bits of x are >= those of y (no borrow crosses a byte), so x < y is bit 7 of
// (~x & y) | ~((x ^ y) | t).  The counts stay <= 121 < 128, and (H + rank - count) has bit 7 set where count <= rank, that is
// where element `rank` of the sorted window is >= the trial value: the trial bit stays.
template <int C, int K>
__device__ __forceinline__ void ph_median_select(const uint32_t *base, int pitch, uint32_t *out)
{
    constexpr int N = ((4 + K - 1) * C + 3) / 4;                        // dwords of one window row that a lane needs
    constexpr uint32_t H = 0x80808080u, ONES = 0x01010101u, RANK = (K * K - 1) / 2;
    uint32_t res[C];
#pragma unroll
    for (int m = 0; m < C; ++m) res[m] = 0;
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
        uint32_t trial[C], tl[C], cnt[C];
#pragma unroll
        for (int m = 0; m < C; ++m) { trial[m] = res[m] | (ONES << bit); tl[m] = trial[m] & ~H; cnt[m] = 0; }
#pragma unroll 1
        for (int r = 0; r < K; ++r) {
            uint32_t row[N];
#pragma unroll
            for (int i = 0; i < N; ++i) row[i] = base[r * pitch + i];
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int m = 0; m < C; ++m) {
                    const int off = 4 * m + j * C, i = off >> 2, s = off & 3;
                    const uint32_t x = s ? __builtin_amdgcn_alignbyte(row[i + 1 < N ? i + 1 : i], row[i], (uint32_t)s) : row[i];
                    const uint32_t t = (x | H) - tl[m];
                    const uint32_t lt = ((~x & trial[m]) | ~((x ^ trial[m]) | t)) & H;
                    cnt[m] += lt >> 7;
                }
        }
#pragma unroll
        for (int m = 0; m < C; ++m) res[m] |= (((H + RANK * ONES) - cnt[m]) & H) >> (7 - bit);
    }
#pragma unroll
    for (int m = 0; m < C; ++m) out[m] = res[m];
}

template <int C>
__global__ __launch_bounds__(PH_THREADS) void photo_median_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, ph_launch L)
{
    typedef ph_med_shape<C> S;
    __shared__ __attribute__((aligned(16))) uint32_t tile[(PH_TH + 2 * PH_MED_HALO) * S::PITCH];
    int b = 0;
    for (int i = 1; i < L.m; ++i)
        if ((int)blockIdx.x >= L.img[i].block0) b = i;
    const ph_image &d = L.img[b];
    const int t = (int)blockIdx.x - d.block0;
    const int ty0 = (t / d.tiles_x) * PH_TH, tx0 = (t - (t / d.tiles_x) * d.tiles_x) * PH_TW;
    const int w = d.w, h = d.h, kk = d.p[0], rad = kk >> 1, tid = threadIdx.x;
    const int rows = PH_TH + 2 * rad, cols = PH_TW + 2 * rad;
    const uint8_t *s = src + d.src_off;
    uint8_t *tb = (uint8_t *)tile;
    // ---- fill: tile + halo, coordinates clamped to the image (replicate border)
    for (int i = tid; i < rows * cols; i += PH_THREADS) {
        const int ly = i / cols, lx = i - ly * cols;
        const int sy = min(max(ty0 - rad + ly, 0), h - 1), sx = min(max(tx0 - rad + lx, 0), w - 1);
        const uint8_t *p = s + ((int64_t)sy * w + sx) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) tb[ly * (S::PITCH * 4) + lx * C + ch] = p[ch];
    }
    __syncthreads();
    const int ly = tid / (PH_TW / PH_PX), x4 = (tid - ly * (PH_TW / PH_PX)) * PH_PX;
    const int y = ty0 + ly, x = tx0 + x4;
    if (y >= h || x >= w) return;
    union { uint8_t bytes[PH_PX * C]; uint32_t words[C]; } o;
    const uint32_t *base = tile + ly * S::PITCH + (x4 * C) / 4;         // x4 C is a multiple of 4
    switch (kk) {
    case 3: ph_median_select<C, 3>(base, S::PITCH, o.words); break;
    case 5: ph_median_select<C, 5>(base, S::PITCH, o.words); break;
    case 7: ph_median_select<C, 7>(base, S::PITCH, o.words); break;
    case 9: ph_median_select<C, 9>(base, S::PITCH, o.words); break;
    default: ph_median_select<C, 11>(base, S::PITCH, o.words); break;
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

// --------------------------------------------------------------------------------------------------------------- ELASTIC
__device__ __forceinline__ uint32_t ph_pack16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ int ph_lo16(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
__device__ __forceinline__ int ph_hi16(uint32_t v) { return (int)v >> 16; }

template <int C>
__global__ __launch_bounds__(PH_THREADS) void photo_elastic_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, ph_launch L)
{
    __shared__ uint32_t raw[(PH_TH + 2) * PH_EL_RAW_PITCH];             // (ey << 16) | (ex & 0xffff), tile + one ring
    __shared__ uint32_t rsm[(PH_TH + 2) * PH_EL_ROW_PITCH];             // after the row pass, the tile's columns
    int b = 0;
    for (int i = 1; i < L.m; ++i)
        if ((int)blockIdx.x >= L.img[i].block0) b = i;
    const ph_image &d = L.img[b];
    const int t = (int)blockIdx.x - d.block0;
    const int ty0 = (t / d.tiles_x) * PH_TH, tx0 = (t - (t / d.tiles_x) * d.tiles_x) * PH_TW;
    const int w = d.w, h = d.h, aq = d.p[0], w0 = d.p[1], w1 = d.p[2], tid = threadIdx.x;
    // ---- the raw field of the tile plus one ring: Q15 in (-1, 1) inside the image, 0 outside
    for (int i = tid; i < (PH_TH + 2) * (PH_TW + 2); i += PH_THREADS) {
        const int ly = i / (PH_TW + 2), lx = i - ly * (PH_TW + 2);
        const int y = ty0 - 1 + ly, x = tx0 - 1 + lx;
        uint32_t v = 0;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            uint32_t r[4];
            ph_philox((uint32_t)(y * w + x), 0, d.seed, r);             // y w + x < 2^31
            v = ph_pack16((int)(r[0] >> 16) - 32768, (int)(r[1] >> 16) - 32768);
        }
        raw[ly * PH_EL_RAW_PITCH + lx] = v;
    }
    __syncthreads();
    // ---- row pass: |w1 (a + c) + w0 b + 8192| <= 16384 32768 + 8192 < 2^30; the result is back in -32768..32767
    for (int i = tid; i < (PH_TH + 2) * PH_TW; i += PH_THREADS) {
        const int ly = i / PH_TW, lx = i - ly * PH_TW;
        const uint32_t a = raw[ly * PH_EL_RAW_PITCH + lx], m = raw[ly * PH_EL_RAW_PITCH + lx + 1], c = raw[ly * PH_EL_RAW_PITCH + lx + 2];
        const int tx = (w1 * (ph_lo16(a) + ph_lo16(c)) + w0 * ph_lo16(m) + 8192) >> 14;
        const int ty = (w1 * (ph_hi16(a) + ph_hi16(c)) + w0 * ph_hi16(m) + 8192) >> 14;
        rsm[ly * PH_EL_ROW_PITCH + lx] = ph_pack16(tx, ty);
    }
    __syncthreads();
    const int ly = tid / (PH_TW / PH_PX), x4 = (tid - ly * (PH_TW / PH_PX)) * PH_PX;
    const int y = ty0 + ly, x0 = tx0 + x4;
    if (y >= h || x0 >= w) return;
    const uint8_t *s = src + d.src_off;
    union { uint8_t bytes[PH_PX * C]; uint32_t words[C]; } o;
#pragma unroll
    for (int k = 0; k < PH_PX; ++k) {
        const int x = x0 + k;
        // ---- column pass, the displacement in 1 / 32 pixel (|aq s| <= 2^27), the source position and its phase
        const uint32_t a = rsm[ly * PH_EL_ROW_PITCH + x4 + k], m = rsm[(ly + 1) * PH_EL_ROW_PITCH + x4 + k],
                       c = rsm[(ly + 2) * PH_EL_ROW_PITCH + x4 + k];
        const int sx = (w1 * (ph_lo16(a) + ph_lo16(c)) + w0 * ph_lo16(m) + 8192) >> 14;
        const int sy = (w1 * (ph_hi16(a) + ph_hi16(c)) + w0 * ph_hi16(m) + 8192) >> 14;
        const int X = 32 * x + ((aq * sx + (1 << 17)) >> 18), Y = 32 * y + ((aq * sy + (1 << 17)) >> 18);
        const int ix = X >> 5, iy = Y >> 5;
        int wx[4], wy[4];
        ph_keys(X & 31, wx);
        ph_keys(Y & 31, wy);
        int64_t acc[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[ch] = (int64_t)1 << 33;
        if (x < w) {                                                    // the lanes past the row's end store nothing
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = iy - 1 + j;
                if (yy < 0 || yy >= h) continue;                        // a tap outside the image contributes 0
                int inner[C];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) inner[ch] = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xx = ix - 1 + i;
                    if (xx < 0 || xx >= w) continue;
                    const uint8_t *p = s + ((int64_t)yy * w + xx) * C;
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) inner[ch] += wx[i] * (int)p[ch];      // |row sum| < 2^26
                }
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[ch] += (int64_t)wy[j] * inner[ch];
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const int64_t v = acc[ch] >> 34;
            o.bytes[k * C + ch] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
    uint8_t *q = dst + d.dst_off + ((int64_t)y * w + x0) * C;
    const int cnt = w - x0 < PH_PX ? w - x0 : PH_PX;
    if (cnt == PH_PX && (((uintptr_t)q) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < C; ++k) ((uint32_t *)q)[k] = o.words[k];
    } else {
#pragma unroll
        for (int k = 0; k < PH_PX * C; ++k)
            if (k < cnt * C) q[k] = o.bytes[k];
    }
}

// the kernel that runs a mode: 0 photo_point_kernel, 1 photo_tile_kernel, 2 photo_median_kernel, 3 photo_elastic_kernel
static inline int ph_class(int mode)
{
    if (mode == UBD_PHOTO_AFFINE || mode == UBD_PHOTO_GREY || mode == UBD_PHOTO_NOISE || mode == UBD_PHOTO_DROPOUT || mode == UBD_PHOTO_HSV) return 0;
    if (mode == UBD_PHOTO_MEDIAN) return 2;
    if (mode == UBD_PHOTO_ELASTIC) return 3;
    return 1;
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
        UBD_REQUIRE((d.mode >= UBD_PHOTO_AFFINE && d.mode <= UBD_PHOTO_DROPOUT) || (d.mode >= UBD_PHOTO_MEDIAN && d.mode <= UBD_PHOTO_ELASTIC),
                    "ubd_photometric_images: image %d has mode %d (0 affine, 1 grey, 2 filter3, 3 sep, 4 box, 5 noise, 6 dropout, 16 median, "
                    "17 hsv, 18 elastic)", i, d.mode);
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
        if (ph_class(d.mode) == 0)
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
        if (d.mode == UBD_PHOTO_MEDIAN)
            UBD_REQUIRE(d.p[0] >= 3 && d.p[0] <= 2 * PH_MED_HALO + 1 && (d.p[0] & 1), "ubd_photometric_images: image %d: median size %d, must be odd and 3..%d",
                        i, d.p[0], 2 * PH_MED_HALO + 1);
        if (d.mode == UBD_PHOTO_HSV) {
            UBD_REQUIRE(channels == 3, "ubd_photometric_images: image %d: mode 17 (hsv) needs 3 channels, got %d", i, channels);
            UBD_REQUIRE(d.p[0] >= -255 && d.p[0] <= 255 && d.p[1] >= -255 && d.p[1] <= 255,
                        "ubd_photometric_images: image %d: dh = %d, ds = %d, both must be -255..255", i, d.p[0], d.p[1]);
        }
        if (d.mode == UBD_PHOTO_ELASTIC) {
            UBD_REQUIRE(d.p[0] >= 0 && d.p[0] <= 4096, "ubd_photometric_images: image %d: elastic alpha %d (Q8), must be 0..4096", i, d.p[0]);
            UBD_REQUIRE(d.p[1] >= 0 && d.p[2] >= 0 && (int64_t)d.p[1] + 2 * (int64_t)d.p[2] == 16384,
                        "ubd_photometric_images: image %d: elastic taps w0 = %d, w1 = %d, must be >= 0 with w0 + 2 w1 = 16384", i, d.p[1], d.p[2]);
        }
        if (d.mode == UBD_PHOTO_NOISE) {
            float scale;
            memcpy(&scale, &d.p[0], 4);
            UBD_REQUIRE(std::isfinite(scale) && scale >= 0.f, "ubd_photometric_images: image %d: noise scale must be finite and >= 0", i);
        }
    }
    // four passes over the descriptors, one per kernel (ph_class): the pointwise images, the filter tiles, the medians, the
    // elastic gathers; PH_MAX_IMGS per launch
    for (int pass = 0; pass < 4; ++pass) {
        int i = 0;
        while (i < n) {
            ph_launch L{};
            int64_t blocks = 0;
            int m = 0;
            for (; i < n && m < PH_MAX_IMGS; ++i) {
                const ubd_photo_desc &d = descs[i];
                if (ph_class(d.mode) != pass) continue;
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
            } else if (pass == 1) {
                if (channels == 3)
                    hipLaunchKernelGGL(photo_tile_kernel<3>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
                else
                    hipLaunchKernelGGL(photo_tile_kernel<1>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
            } else if (pass == 2) {
                if (channels == 3)
                    hipLaunchKernelGGL(photo_median_kernel<3>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
                else
                    hipLaunchKernelGGL(photo_median_kernel<1>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
            } else {
                if (channels == 3)
                    hipLaunchKernelGGL(photo_elastic_kernel<3>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
                else
                    hipLaunchKernelGGL(photo_elastic_kernel<1>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, (hipStream_t)stream, src, dst, L);
            }
            UBD_CHECK_HIP(hipGetLastError());
        }
    }
    return 0;
}
