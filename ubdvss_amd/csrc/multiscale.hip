// The multi-scale model for gfx950, inference and training: the reference's NetManager._build_multiscale_model (net.py:44-59, :368-389) runs the base net on the
// batch at full, 1/2, ..., 1/2^P size, brings every result back to the full map size with UpSampling2D (nearest) and averages them.
//
// Pyramid.  The reference resizes with tf.image.resize_images (TF1's legacy bilinear, align_corners=False): in = out_index *
// (in_size / out_size), lo = floor(in), hi = min(ceil(in), in_size - 1), lerp = in - lo.  The maps of the levels can only be combined
// when both sides are multiples of 4 * 2^P; then in_size / out_size is exactly 2^s, `in` is an integer, lerp is 0 and -- for finite
// inputs -- the resize is the plain decimation x[:, ::2^s, ::2^s, :] (tests/test_multiscale_host.py holds the general
// formula against the slice).  Decimation commutes with the per-pixel preprocessing, so uint8 pixels stay uint8 and every level's
// forward pass fuses the preprocessing into its first layer as usual.
//
// Gather kernel: ONE launch writes levels 1..P, packed one after another.  Every tap of level s + 1 is a tap of level s, so a thread
// loads one piece of an EVEN source row once (16 bytes per channel; lanes of a wave read one contiguous run) and stores the piece's
// taps to every level the row belongs to; odd rows are never read.  A piece is PX pixels, PX dividing the row width (16 or 8 uint8
// pixels, 4 floats: the width is a multiple of 8), so there is no row tail: nothing is read or written outside a row.
//
// Fuse kernel: out = (y_0 + y_1[i >> 1, j >> 1] + ... + y_P[i >> P, j >> P]) / (P + 1) per channel, in fp32, added in level order,
// then ONE IEEE division (no reciprocal; the unit is built with -ffp-contract=off, and nothing here could contract anyway).  Level 0
// is read once with 8- or 16-byte loads; the coarser levels are re-read by 4^s neighbours and come from cache.  `out` may alias y_0:
// a thread reads exactly the elements it writes, before it writes them.  Parity with the reduction order of TF's K.mean is unpinned.
//
// ubd_forward_multiscale chains gather -> ubd_forward at level 0 (which packs the weights) -> ubd_forward at levels 1..P on the same
// workspace with UBD_IN_PREPACKED -> fuse, all on the caller's stream: no synchronisation, no allocation, no host read, a strictly
// linear chain that a HIP graph captures as it is.
//
// Training (ubd_train_step_multiscale).  The adjoint of the fuse: level s receives S_s / (P + 1), S_0 = dmean and S_s the 2 x 2 sums of
// S_(s-1), (a + b) + (c + d) per channel.  ONE launch: a block takes a tile of 2^P map rows x a run of whole coarsest cells, reads its
// piece of dmean once (the widest loads the addresses allow), keeps it in LDS and folds it level by level between two LDS buffers
// (level s reads s - 1 from one and writes the other; the sizes shrink by four); every level's quotient leaves from the lane that
// formed the sum -- no atomics, nothing read back from global memory.  Lanes run along (pixel, channel) of a level's row, so the four
// partners sit at +k, +row, +row + k floats: b32 reads at stride 2 for k = 1 (two-way bank conflict, on a kernel that moves one map).
// The chain: gather -> per level the training forward (all activations kept, in the level's own train_layout region) -> fuse -> loss
// on the mean map -> fuse adjoint -> per level the backward pass into the level's own gradient vector -> one kernel that adds the
// vectors in level order.  Each level packs its own weight fragments, exactly as ubd_train_step does for its shape.
#include <optional>
#include "bwd_common.h"

#define MS_MAX_POWER 4

template <int BYTES> struct ms_unit;
template <> struct ms_unit<1> { typedef unsigned char type; };
template <> struct ms_unit<2> { typedef unsigned short type; };
template <> struct ms_unit<4> { typedef unsigned type; };
template <> struct ms_unit<8> { typedef uint2 type; };
template <> struct ms_unit<16> { typedef uint4 type; };

// Keeps a loaded piece whole: only every second pixel of it is used, and hipcc otherwise narrows the 16-byte load into one byte /
// short load per tap (13 byte loads in the uint8 kernels).  No instruction; the value just becomes opaque.
__device__ __forceinline__ void ms_keep(unsigned &u) { asm volatile("" : "+v"(u)); }
__device__ __forceinline__ void ms_keep(uint2 &u) { asm volatile("" : "+v"(u.x), "+v"(u.y)); }
__device__ __forceinline__ void ms_keep(uint4 &u) { asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w)); }

struct ms_levels { unsigned char *p[MS_MAX_POWER + 1]; };     // p[s]: level s of the packed buffer (p[0] unused)

// taps of level S inside one piece of PX pixels (v) of source row y, piece index `piece` of the row
template <typename T, int C, int PX, int S>
__device__ __forceinline__ void ms_emit(const T (&v)[PX * C], unsigned char *level, size_t img, int y, int piece, int H, int W)
{
    const int hs = H >> S, ws = W >> S;
    unsigned char *row = level + ((img * hs + (size_t)(y >> S)) * ws) * (C * sizeof(T));
    if constexpr ((PX >> S) >= 1) {
        constexpr int Q = PX >> S;                            // pixels of this level in the piece
        T o[Q * C];
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int c = 0; c < C; ++c) o[q * C + c] = v[(q << S) * C + c];
        typedef typename ms_unit<Q * sizeof(T)>::type SU;     // Q * C elements = C stores of Q elements, each aligned to its size
        SU su[C];
        __builtin_memcpy(su, o, sizeof(o));
        SU *d = (SU *)(row + (size_t)piece * (Q * C * sizeof(T)));
#pragma unroll
        for (int j = 0; j < C; ++j) d[j] = su[j];
    } else {
        constexpr int R = (1 << S) / PX;                      // pieces per pixel of this level
        if ((piece & (R - 1)) == 0) {
            T *d = (T *)row + (size_t)(piece / R) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) d[c] = v[c];
        }
    }
}

// block = (tx pieces) x (256 / tx even rows); total_rows = n * H / 2 even source rows
template <typename T, int C, int PX>
__global__ __launch_bounds__(256) void ms_gather_kernel(const unsigned char *__restrict__ src, ms_levels lv, int H, int W, int P,
                                                        unsigned total_rows)
{
    constexpr int LB = PX * sizeof(T);                        // bytes of one load: 16 (8 for uint8 rows whose width is 8 mod 16)
    typedef typename ms_unit<LB>::type LU;
    const int pieces = W / PX;
    const unsigned er = blockIdx.x * blockDim.y + threadIdx.y;
    if (er >= total_rows) return;
    const unsigned rows = (unsigned)H >> 1;
    const size_t img = er / rows;
    const int y = 2 * (int)(er - (unsigned)img * rows);
    const unsigned char *srow = src + ((img * H + (size_t)y) * W) * (C * sizeof(T));
    for (int piece = threadIdx.x; piece < pieces; piece += blockDim.x) {
        const LU *p = (const LU *)(srow + (size_t)piece * (LB * C));
        LU u[C];
#pragma unroll
        for (int j = 0; j < C; ++j) u[j] = p[j];
#pragma unroll
        for (int j = 0; j < C; ++j) ms_keep(u[j]);
        T v[PX * C];
        __builtin_memcpy(v, u, sizeof(v));
        ms_emit<T, C, PX, 1>(v, lv.p[1], img, y, piece, H, W);
        if (P >= 2 && (y & 3) == 0) ms_emit<T, C, PX, 2>(v, lv.p[2], img, y, piece, H, W);
        if (P >= 3 && (y & 7) == 0) ms_emit<T, C, PX, 3>(v, lv.p[3], img, y, piece, H, W);
        if (P >= 4 && (y & 15) == 0) ms_emit<T, C, PX, 4>(v, lv.p[4], img, y, piece, H, W);
    }
}

struct ms_coarse { const float *p[MS_MAX_POWER + 1]; };       // p[s]: level s logits, s = 1..P

// block = (tx groups of VEC floats) x (256 / tx map rows); total_rows = n * mh rows of mw * k floats
template <int VEC>
__global__ __launch_bounds__(256) void ms_fuse_kernel(const float *y0, ms_coarse lv, float *out, int mh, int mw, int k, int P,
                                                      float count, unsigned total_rows)
{
    typedef typename ms_unit<4 * VEC>::type VU;
    const unsigned r = blockIdx.x * blockDim.y + threadIdx.y;
    if (r >= total_rows) return;
    const size_t img = r / (unsigned)mh;
    const int i = (int)(r - (unsigned)img * (unsigned)mh);
    const int row_len = mw * k;
    const size_t row0 = (size_t)r * row_len;
    size_t base[MS_MAX_POWER + 1];                            // first float of row i >> s of level s
#pragma unroll
    for (int s = 1; s <= MS_MAX_POWER; ++s)
        base[s] = s <= P ? ((img * (size_t)(mh >> s) + (size_t)(i >> s)) * (size_t)(mw >> s)) * k : 0;
    for (int e = threadIdx.x * VEC; e < row_len; e += blockDim.x * VEC) {
        float v[VEC];
        VU u = *(const VU *)(y0 + row0 + e);
        __builtin_memcpy(v, &u, sizeof(v));
        int j = e / k, c = e - j * k;
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
            float acc = v[t];
#pragma unroll
            for (int s = 1; s <= MS_MAX_POWER; ++s)
                if (s <= P) acc = acc + lv.p[s][base[s] + (size_t)(j >> s) * k + c];
            v[t] = acc / count;
            if (++c == k) { c = 0; ++j; }
        }
        __builtin_memcpy(&u, v, sizeof(v));
        *(VU *)(out + row0 + e) = u;
    }
}


// ------------------------------------------------------------------------------------ adjoint of the fuse
#define MSB_TILE_FLOATS 8192                                  // level 0 of a block's tile: at least one coarsest cell, 4^4 pixels x 32 channels
struct ms_grad_levels { float *p[MS_MAX_POWER + 1]; };        // p[s]: level s of the packed gradients

// block b = (tile row = image x row of coarsest cells, chunk of cw_pix level-0 pixels); rows of a tile: 2^P
template <int VEC>
__global__ __launch_bounds__(256) void ms_fuse_bwd_kernel(const float *__restrict__ dmean, ms_grad_levels lv, int mh, int mw, int k, int P,
                                                          float count, int cw_pix, int nchunks)
{
    typedef typename ms_unit<4 * VEC>::type VU;
    __shared__ __attribute__((aligned(16))) float s_a[MSB_TILE_FLOATS];       // levels 0, 2, 4
    __shared__ __attribute__((aligned(16))) float s_b[MSB_TILE_FLOATS / 4];   // levels 1, 3
    const unsigned chunk = blockIdx.x % (unsigned)nchunks, tr = blockIdx.x / (unsigned)nchunks;
    const unsigned cell_rows = (unsigned)mh >> P;
    const size_t img = tr / cell_rows;
    const int ti = (int)(tr - (unsigned)img * cell_rows);
    const int pix0 = (int)chunk * cw_pix, wpix = min(cw_pix, mw - pix0);      // both multiples of 2^P
    const int TR = 1 << P, wid0 = wpix * k;
    for (int e = threadIdx.x * VEC; e < TR * wid0; e += 256 * VEC) {          // wid0 is a multiple of VEC: a vector stays in its row
        const int r = e / wid0, q = e - r * wid0;
        const size_t g = ((img * mh + (size_t)(ti * TR + r)) * mw + pix0) * k + q;
        VU u = *(const VU *)(dmean + g);
        *(VU *)(s_a + e) = u;
        float v[VEC];
        __builtin_memcpy(v, &u, sizeof(v));
#pragma unroll
        for (int t = 0; t < VEC; ++t) v[t] = v[t] / count;
        __builtin_memcpy(&u, v, sizeof(v));
        *(VU *)(lv.p[0] + g) = u;
    }
    for (int s = 1; s <= P; ++s) {
        __syncthreads();
        const float *src = (s & 1) ? s_a : s_b;
        float *dst = (s & 1) ? s_b : s_a;
        const int rows = TR >> s, wid = wid0 >> s;                            // this level's tile: rows x (wpix >> s) pixels x k
        const size_t g0 = ((img * (size_t)(mh >> s) + (size_t)(ti * rows)) * (size_t)(mw >> s) + (size_t)(pix0 >> s)) * k;
        const size_t grow = (size_t)(mw >> s) * k;
        for (int e = threadIdx.x; e < rows * wid; e += 256) {
            const int r = e / wid, q = e - r * wid, j = q / k, c = q - j * k;
            const float *t = src + 4 * r * wid + 2 * j * k + c;               // row 2 r of level s - 1 (2 wid floats long), pixel 2 j
            const float v = (t[0] + t[k]) + (t[2 * wid] + t[2 * wid + k]);
            dst[e] = v;
            lv.p[s][g0 + (size_t)r * grow + q] = v / count;
        }
    }
}

// grads = ((g_0 + g_1) + g_2) + ... + g_P, the levels' gradient vectors `stride` floats apart
__global__ __launch_bounds__(256) void ms_grad_sum_kernel(const float *__restrict__ g, size_t stride, int levels, float *__restrict__ out,
                                                          size_t count)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float acc = g[i];
    for (int s = 1; s < levels; ++s) acc = acc + g[s * stride + i];
    out[i] = acc;
}

// ------------------------------------------------------------------------------------ host
static bool ms_power_ok(int P) { return P >= 0 && P <= MS_MAX_POWER; }

// block shape for rows of `items` work items: tx = the power of two that covers a row (at most 256), 256 / tx rows per block
static void ms_block_shape(long items, unsigned total_rows, dim3 *grid, dim3 *block)
{
    unsigned tx = 1;
    while (tx < 256 && (long)tx < items) tx <<= 1;
    const unsigned ty = 256 / tx;
    *block = dim3(tx, ty);
    *grid = dim3((total_rows + ty - 1) / ty);
}

extern "C" size_t ubd_multiscale_levels_bytes(int n, int height, int width, int pixel_bytes, int first_level, int max_scale_power)
{
    if (n < 1 || height < 1 || width < 1 || pixel_bytes < 1 || !ms_power_ok(max_scale_power) || first_level < 0) return 0;
    const int m = 1 << max_scale_power;
    if (height % m || width % m) return 0;
    size_t total = 0;
    for (int s = first_level; s <= max_scale_power; ++s) total += (size_t)n * (height >> s) * (width >> s) * pixel_bytes;
    return total;
}

static int ms_check_sides(const char *fn, int n, int height, int width, int P)
{
    UBD_REQUIRE(ms_power_ok(P), "%s: max_scale_power %d outside 0..%d", fn, P, MS_MAX_POWER);
    const int m = 4 << P;
    UBD_REQUIRE(n > 0 && height > 0 && width > 0 && height % m == 0 && width % m == 0,
                "%s: height and width must be positive multiples of %d (4 * 2^max_scale_power, max_scale_power = %d), got %d x %d", fn, m, P,
                height, width);
    return 0;
}

template <typename T, int C>
static void ms_launch_gather(const void *images, const ms_levels &lv, int n, int H, int W, int P, hipStream_t st)
{
    const unsigned total_rows = (unsigned)n * (unsigned)(H / 2);
    dim3 grid, block;
    if constexpr (sizeof(T) == 1) {
        if (W % 16 == 0) {
            ms_block_shape(W / 16, total_rows, &grid, &block);
            hipLaunchKernelGGL((ms_gather_kernel<T, C, 16>), grid, block, 0, st, (const unsigned char *)images, lv, H, W, P, total_rows);
        } else {
            ms_block_shape(W / 8, total_rows, &grid, &block);
            hipLaunchKernelGGL((ms_gather_kernel<T, C, 8>), grid, block, 0, st, (const unsigned char *)images, lv, H, W, P, total_rows);
        }
    } else {
        ms_block_shape(W / 4, total_rows, &grid, &block);
        hipLaunchKernelGGL((ms_gather_kernel<T, C, 4>), grid, block, 0, st, (const unsigned char *)images, lv, H, W, P, total_rows);
    }
}

extern "C" int ubd_multiscale_gather(const void *images, int in_dtype, int n, int height, int width, int channels, int max_scale_power,
                                     void *levels_out, size_t levels_bytes, void *stream)
{
    UBD_REQUIRE(images && levels_out, "ubd_multiscale_gather: null argument");
    UBD_REQUIRE(in_dtype == UBD_IN_F32 || in_dtype == UBD_IN_U8, "ubd_multiscale_gather: bad in_dtype %d", in_dtype);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_multiscale_gather: channels must be 1 or 3, got %d", channels);
    if (int rc = ms_check_sides("ubd_multiscale_gather", n, height, width, max_scale_power)) return rc;
    UBD_REQUIRE(max_scale_power >= 1, "ubd_multiscale_gather: max_scale_power 0 has no levels to write");
    UBD_REQUIRE((size_t)n * (height / 2) < (1ull << 31), "ubd_multiscale_gather: n * height / 2 must stay below 2^31");
    UBD_REQUIRE(((uintptr_t)images & 15) == 0 && ((uintptr_t)levels_out & 15) == 0,
                "ubd_multiscale_gather: images and levels_out must be 16-byte aligned");
    const int pixel_bytes = channels * (in_dtype == UBD_IN_U8 ? 1 : 4);
    const size_t need = ubd_multiscale_levels_bytes(n, height, width, pixel_bytes, 1, max_scale_power);
    UBD_REQUIRE(levels_bytes >= need, "ubd_multiscale_gather: levels buffer too small (%zu < %zu)", levels_bytes, need);
    ms_levels lv;
    memset(&lv, 0, sizeof(lv));
    for (int s = 1; s <= max_scale_power; ++s)
        lv.p[s] = (unsigned char *)levels_out + ubd_multiscale_levels_bytes(n, height, width, pixel_bytes, 1, s - 1);
    const hipStream_t st = (hipStream_t)stream;
    if (in_dtype == UBD_IN_U8) {
        if (channels == 1) ms_launch_gather<unsigned char, 1>(images, lv, n, height, width, max_scale_power, st);
        else ms_launch_gather<unsigned char, 3>(images, lv, n, height, width, max_scale_power, st);
    } else {
        if (channels == 1) ms_launch_gather<float, 1>(images, lv, n, height, width, max_scale_power, st);
        else ms_launch_gather<float, 3>(images, lv, n, height, width, max_scale_power, st);
    }
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}

// y0: level 0; coarse: levels 1..P packed; out may be y0
static int ms_fuse(const char *fn, const float *y0, const float *coarse, int n, int mh, int mw, int k, int P, float *out, hipStream_t st)
{
    UBD_REQUIRE(ms_power_ok(P), "%s: max_scale_power %d outside 0..%d", fn, P, MS_MAX_POWER);
    const int m = 1 << P;
    UBD_REQUIRE(n > 0 && mh > 0 && mw > 0 && mh % m == 0 && mw % m == 0,
                "%s: map height and width must be positive multiples of %d (2^max_scale_power), got %d x %d", fn, m, mh, mw);
    UBD_REQUIRE(k >= 1 && k <= UBD_MAX_CLASSES + 1, "%s: k must be 1..%d, got %d", fn, UBD_MAX_CLASSES + 1, k);
    UBD_REQUIRE((size_t)n * mh < (1ull << 31) && (size_t)mw * k < (1ull << 31), "%s: n * map_h and map_w * k must stay below 2^31", fn);
    UBD_REQUIRE((((uintptr_t)y0 | (uintptr_t)coarse | (uintptr_t)out) & 3) == 0, "%s: misaligned argument", fn);
    ms_coarse lv;
    memset(&lv, 0, sizeof(lv));
    for (int s = 1; s <= P; ++s) lv.p[s] = coarse + ubd_multiscale_levels_bytes(n, mh, mw, k * 4, 1, s - 1) / 4;
    const unsigned total_rows = (unsigned)n * (unsigned)mh;
    const int row_len = mw * k;
    const bool a16 = (((uintptr_t)y0 | (uintptr_t)out) & 15) == 0, a8 = (((uintptr_t)y0 | (uintptr_t)out) & 7) == 0;
    const int vec = (a16 && row_len % 4 == 0) ? 4 : (a8 && row_len % 2 == 0) ? 2 : 1;      // every row then starts on a whole vector
    dim3 grid, block;
    ms_block_shape(row_len / vec, total_rows, &grid, &block);
    const float count = (float)(P + 1);
    if (vec == 4) hipLaunchKernelGGL(ms_fuse_kernel<4>, grid, block, 0, st, y0, lv, out, mh, mw, k, P, count, total_rows);
    else if (vec == 2) hipLaunchKernelGGL(ms_fuse_kernel<2>, grid, block, 0, st, y0, lv, out, mh, mw, k, P, count, total_rows);
    else hipLaunchKernelGGL(ms_fuse_kernel<1>, grid, block, 0, st, y0, lv, out, mh, mw, k, P, count, total_rows);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int ubd_multiscale_fuse(const float *level_logits, int n, int map_h, int map_w, int k, int max_scale_power, float *out,
                                   void *stream)
{
    UBD_REQUIRE(level_logits && out, "ubd_multiscale_fuse: null argument");
    UBD_REQUIRE(n > 0 && map_h > 0 && map_w > 0 && k > 0, "ubd_multiscale_fuse: sizes must be positive");
    return ms_fuse("ubd_multiscale_fuse", level_logits, level_logits + (size_t)n * map_h * map_w * k, n, map_h, map_w, k, max_scale_power,
                   out, (hipStream_t)stream);
}

extern "C" int ubd_multiscale_fuse_backward(const float *dmean, int n, int map_h, int map_w, int k, int max_scale_power,
                                            float *level_dlogits, void *stream)
{
    const char *fn = "ubd_multiscale_fuse_backward";
    const int P = max_scale_power;
    UBD_REQUIRE(dmean && level_dlogits, "%s: null argument", fn);
    UBD_REQUIRE(n > 0 && map_h > 0 && map_w > 0 && k > 0, "%s: sizes must be positive", fn);
    UBD_REQUIRE(ms_power_ok(P), "%s: max_scale_power %d outside 0..%d", fn, P, MS_MAX_POWER);
    const int m = 1 << P;
    UBD_REQUIRE(map_h % m == 0 && map_w % m == 0,
                "%s: map height and width must be positive multiples of %d (2^max_scale_power), got %d x %d", fn, m, map_h, map_w);
    UBD_REQUIRE(k <= UBD_MAX_CLASSES + 1, "%s: k must be 1..%d, got %d", fn, UBD_MAX_CLASSES + 1, k);
    UBD_REQUIRE((size_t)n * map_h < (1ull << 31) && (size_t)map_w * k < (1ull << 31), "%s: n * map_h and map_w * k must stay below 2^31", fn);
    UBD_REQUIRE((((uintptr_t)dmean | (uintptr_t)level_dlogits) & 3) == 0, "%s: misaligned argument", fn);
    // a block's tile: 2^P rows x `cw` coarsest cells, about 4096 floats of level 0 and never more than MSB_TILE_FLOATS (one cell of
    // 4^4 pixels x 32 channels); a row cut into several chunks is cut at multiples of four cells, so that every chunk starts on a whole vector
    const int cells = map_w >> P;
    const size_t per_cell = ((size_t)1 << (2 * P)) * k;
    int cw = (int)std::min<size_t>(cells, std::max<size_t>(1, 4096 / per_cell));
    if (cw < cells && cw >= 4) cw &= ~3;
    const int cw_pix = cw << P, nchunks = (cells + cw - 1) / cw;
    const size_t blocks = (size_t)n * (map_h >> P) * nchunks;
    UBD_REQUIRE(per_cell * cw <= MSB_TILE_FLOATS && blocks < (1ull << 31), "%s: too many tiles (%zu)", fn, blocks);
    const int row_len = map_w * k, chunk_len = cw_pix * k;
    const uintptr_t both = (uintptr_t)dmean | (uintptr_t)level_dlogits;
    const bool v4 = (both & 15) == 0 && row_len % 4 == 0 && (nchunks == 1 || chunk_len % 4 == 0);
    const bool v2 = (both & 7) == 0 && row_len % 2 == 0 && (nchunks == 1 || chunk_len % 2 == 0);
    ms_grad_levels lv;
    memset(&lv, 0, sizeof(lv));
    for (int s = 0; s <= P; ++s) lv.p[s] = level_dlogits + (s ? ubd_multiscale_levels_bytes(n, map_h, map_w, k * 4, 0, s - 1) / 4 : 0);
    const float count = (float)(P + 1);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(256);
    if (v4) hipLaunchKernelGGL(ms_fuse_bwd_kernel<4>, grid, block, 0, st, dmean, lv, map_h, map_w, k, P, count, cw_pix, nchunks);
    else if (v2) hipLaunchKernelGGL(ms_fuse_bwd_kernel<2>, grid, block, 0, st, dmean, lv, map_h, map_w, k, P, count, cw_pix, nchunks);
    else hipLaunchKernelGGL(ms_fuse_bwd_kernel<1>, grid, block, 0, st, dmean, lv, map_h, map_w, k, P, count, cw_pix, nchunks);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}

// workspace of ubd_forward_multiscale: [forward workspace of the largest level | levels 1..P of the images | logits of levels 1..P]
struct ms_layout { size_t fwd, off_images, off_logits, total; };

static int ms_layout_compute(const ubd_handle *h, int in_dtype, int n, int H, int W, int P, ms_layout *L)
{
    size_t fwd = 0;
    for (int s = 0; s <= P; ++s) {
        const size_t b = ubd_forward_workspace_bytes(h, n, H >> s, W >> s);
        if (b > fwd) fwd = b;
    }
    L->fwd = fwd;
    size_t off = ubd_align_up(fwd, 256);
    L->off_images = off;
    if (P >= 1) off += ubd_align_up(ubd_multiscale_levels_bytes(n, H, W, h->cfg.c_in * (in_dtype == UBD_IN_U8 ? 1 : 4), 1, P), 256);
    L->off_logits = off;
    if (P >= 1) off += ubd_align_up(ubd_multiscale_levels_bytes(n, H / 4, W / 4, h->k_out * 4, 1, P), 256);
    L->total = P >= 1 ? off : fwd;
    return 0;
}

extern "C" size_t ubd_forward_multiscale_workspace_bytes(const ubd_handle *h, int in_dtype, int n, int height, int width, int max_scale_power)
{
    const int dt = in_dtype & ~UBD_IN_PREPACKED;
    if (!h || !ms_power_ok(max_scale_power) || n < 1 || height < 1 || width < 1 || (dt != UBD_IN_F32 && dt != UBD_IN_U8)) return 0;
    if (height % (4 << max_scale_power) || width % (4 << max_scale_power)) return 0;
    ms_layout L;
    ms_layout_compute(h, dt, n, height, width, max_scale_power, &L);
    return L.total;
}

extern "C" int ubd_forward_multiscale(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing, int n,
                                      int height, int width, int max_scale_power, float *logits, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    UBD_REQUIRE(h && params && images && logits && workspace, "ubd_forward_multiscale: null argument");
    const int P = max_scale_power;
    const int dt = in_dtype & ~UBD_IN_PREPACKED;
    UBD_REQUIRE(dt == UBD_IN_F32 || dt == UBD_IN_U8, "ubd_forward_multiscale: bad in_dtype %d", in_dtype);
    if (int rc = ms_check_sides("ubd_forward_multiscale", n, height, width, P)) return rc;
    if (P == 0)                                               // the single-scale pass itself: the same launches, the same bytes
        return ubd_forward(h, params, images, in_dtype, preprocessing, n, height, width, logits, workspace, workspace_bytes, stream);
    UBD_REQUIRE(h->cfg.c_in == 1 || h->cfg.c_in == 3, "ubd_forward_multiscale: the pyramid needs c_in 1 or 3");
    ms_layout L;
    ms_layout_compute(h, dt, n, height, width, P, &L);
    UBD_REQUIRE(workspace_bytes >= L.total, "ubd_forward_multiscale: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    char *ws = (char *)workspace;
    const int pixel_bytes = h->cfg.c_in * (dt == UBD_IN_U8 ? 1 : 4);
    const int k = h->k_out, mh = height / 4, mw = width / 4;
    if (int rc = ubd_multiscale_gather(images, dt, n, height, width, h->cfg.c_in, P, ws + L.off_images, L.off_logits - L.off_images, stream))
        return rc;
    // level 0 writes `logits` (the fuse then runs in place) and packs the weights unless the caller vouches for them; the other levels
    // find the fragments at the head of the same workspace
    if (int rc = ubd_forward(h, params, images, in_dtype, preprocessing, n, height, width, logits, ws, L.fwd, stream)) return rc;
    for (int s = 1; s <= P; ++s) {
        const char *x = ws + L.off_images + ubd_multiscale_levels_bytes(n, height, width, pixel_bytes, 1, s - 1);
        float *y = (float *)(ws + L.off_logits + ubd_multiscale_levels_bytes(n, mh, mw, k * 4, 1, s - 1));
        if (int rc = ubd_forward(h, params, x, dt | UBD_IN_PREPACKED, preprocessing, n, height >> s, width >> s, y, ws, L.fwd, stream)) return rc;
    }
    return ms_fuse("ubd_forward_multiscale", logits, (const float *)(ws + L.off_logits), n, mh, mw, k, P, logits, (hipStream_t)stream);
}

// workspace of ubd_train_step_multiscale (P >= 1): [train_layout region of level 0 | ... | of level P | levels 1..P of the images |
// logits of levels 0..P | mean map | d loss / d mean | d logits of levels 0..P | gradient vectors of levels 0..P]
struct mst_layout {
    train_layout T[MS_MAX_POWER + 1];
    size_t off_level[MS_MAX_POWER + 1], off_images, off_logits, off_mean, off_dmean, off_dlogits, off_grads, grad_stride, total;
};

static void mst_layout_compute(const ubd_handle *h, int in_dtype, int n, int H, int W, int P, mst_layout *L)
{
    size_t off = 0;
    for (int s = 0; s <= P; ++s) {
        ubd_train_layout_compute(h, n, H >> s, W >> s, &L->T[s]);
        L->off_level[s] = off;
        off += ubd_align_up(L->T[s].total, 256);
    }
    const size_t maps = ubd_align_up(ubd_multiscale_levels_bytes(n, H / 4, W / 4, h->k_out * 4, 0, P), 256);
    const size_t map0 = ubd_align_up((size_t)n * (H / 4) * (W / 4) * h->k_out * 4, 256);
    L->off_images = off;  off += ubd_align_up(ubd_multiscale_levels_bytes(n, H, W, h->cfg.c_in * (in_dtype == UBD_IN_U8 ? 1 : 4), 1, P), 256);
    L->off_logits = off;  off += maps;
    L->off_mean = off;    off += map0;
    L->off_dmean = off;   off += map0;
    L->off_dlogits = off; off += maps;
    L->grad_stride = ubd_align_up(h->n_params * sizeof(float), 256) / sizeof(float);
    L->off_grads = off;   off += (size_t)(P + 1) * L->grad_stride * sizeof(float);
    L->total = off;
}

extern "C" size_t ubd_train_multiscale_workspace_bytes(const ubd_handle *h, int in_dtype, int n, int height, int width, int max_scale_power)
{
    if (!h || !ms_power_ok(max_scale_power) || n < 1 || height < 1 || width < 1 || (in_dtype != UBD_IN_F32 && in_dtype != UBD_IN_U8)) return 0;
    if (height % (4 << max_scale_power) || width % (4 << max_scale_power)) return 0;
    if (max_scale_power == 0) return ubd_train_workspace_bytes(h, n, height, width);
    mst_layout L;
    mst_layout_compute(h, in_dtype, n, height, width, max_scale_power, &L);
    return L.total;
}

extern "C" int ubd_train_step_multiscale(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                                         const int32_t *y_true, int n, int height, int width, int max_scale_power, float *grads,
                                         float *loss, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "ubd_train_step_multiscale";
    UBD_REQUIRE(h && params && images && y_true && grads && loss && workspace, "%s: null argument", fn);
    const int P = max_scale_power;
    if (int rc = ms_check_sides(fn, n, height, width, P)) return rc;
    if (P == 0)                                               // the single-scale step itself: the same launches, the same bytes
        return ubd_train_step(h, params, images, in_dtype, preprocessing, y_true, n, height, width, grads, loss, workspace, workspace_bytes, stream);
    // every level's backward pass would start and finish a gradient exchange of its own on a vector that is not the step's: refused,
    // never skipped.  Without UBD_COMM_FUSED the caller all-reduces `grads` after this call, as after ubd_train_step.
    UBD_REQUIRE(!ubd_comm_fused(h), "%s: the handle's communicator fuses the gradient exchange into ubd_train_step (UBD_COMM_FUSED); the "
                "multi-scale step needs the explicit mode: ubd_comm_init without UBD_COMM_FUSED, then ubd_allreduce_grads after the step", fn);
    UBD_REQUIRE(in_dtype == UBD_IN_F32 || in_dtype == UBD_IN_U8, "%s: bad in_dtype %d", fn, in_dtype);
    UBD_REQUIRE(h->cfg.dtype == UBD_F32 || h->use_wino, "%s: 16-bit activations need the Winograd data-gradient kernel (unset UBD_DILCONV=direct)", fn);
    UBD_REQUIRE(h->cfg.c_in == 1 || h->cfg.c_in == 3, "%s: the pyramid needs c_in 1 or 3", fn);
    UBD_REQUIRE(((uintptr_t)images & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "%s: images and workspace must be 16-byte aligned", fn);
    mst_layout L;
    mst_layout_compute(h, in_dtype, n, height, width, P, &L);
    UBD_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, L.total);
    const hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int pixel_bytes = h->cfg.c_in * (in_dtype == UBD_IN_U8 ? 1 : 4);
    const int k = h->k_out, mh = height / 4, mw = width / 4;
    float *level_logits = (float *)(ws + L.off_logits), *level_dlogits = (float *)(ws + L.off_dlogits);
    float *mean = (float *)(ws + L.off_mean), *dmean = (float *)(ws + L.off_dmean), *level_grads = (float *)(ws + L.off_grads);
    if (int rc = ubd_multiscale_gather(images, in_dtype, n, height, width, h->cfg.c_in, P, ws + L.off_images, L.off_logits - L.off_images, stream))
        return rc;
    std::optional<bwd_pass> pass[MS_MAX_POWER + 1];            // a level's pass: its slice, its region of the workspace, its share of the packed buffers
    for (int s = 0; s <= P; ++s) {
        const size_t map_off = s ? ubd_multiscale_levels_bytes(n, mh, mw, k * 4, 0, s - 1) / 4 : 0;
        const void *x = s ? ws + L.off_images + ubd_multiscale_levels_bytes(n, height, width, pixel_bytes, 1, s - 1) : images;
        pass[s].emplace(bwd_pass{h, params, x, in_dtype, preprocessing, n, height >> s, width >> s, level_dlogits + map_off,
                                 level_grads + (size_t)s * L.grad_stride, ws + L.off_level[s], L.T[s], st});
        if (int rc = ubd_train_forward(*pass[s], level_logits + map_off)) return rc;
    }
    if (int rc = ubd_multiscale_fuse(level_logits, n, mh, mw, k, P, mean, stream)) return rc;
    // the loss scratch is level 0's; not vouched for as zeroed (the bf16 prologue of level 0 did zero it, the call does not rely on it)
    if (int rc = ubd_loss_impl(mean, k, y_true, (long)n * mh * mw, loss, dmean, ws + L.off_level[0] + L.T[0].off_loss, st, h, false)) return rc;
    if (int rc = ubd_multiscale_fuse_backward(dmean, n, mh, mw, k, P, level_dlogits, stream)) return rc;
    for (int s = 0; s <= P; ++s)
        if (int rc = ubd_train_backward(*pass[s])) return rc;
    hipLaunchKernelGGL(ms_grad_sum_kernel, dim3((unsigned)((h->n_params + 255) / 256)), dim3(256), 0, st, level_grads, L.grad_stride, P + 1, grads,
                       (size_t)h->n_params);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
