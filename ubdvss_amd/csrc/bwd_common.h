// What both backward passes of the train step use (bwd32.hip: fp32 gradient tensors; bwd16.hip: bf16 gradient tensors).
//
// Weight gradients: every block writes one row of a partial-sum matrix, reduce_partials_kernel (backward.hip) adds the rows in a
// fixed order into the flat gradient vector (Keras get_weights() order, same as the parameters).
//   head_wgrad   dhk = A9^T dlogits, dhb = sum dlogits                       (MFMA, K-dim = pixels)
#pragma once
#include <algorithm>
#include <type_traits>
#include "common.h"
#include "pack.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Activation element access: the saved forward activations are fp32 (UBD_F32) or 16-bit (UBD_BF16 / UBD_F16);
// gradient tensors between layers are fp32, except in UBD_BF16 mode (bf16: bwd16.h, sepbwd16.h).
template <typename TX> __device__ __forceinline__ float ld_act(const void *base, size_t idx)
{
    return (float)((const TX *)base)[idx];
}
// 16-bit activation modes use every convolution kernel (and the depthwise intermediate) in the activation type
template <typename TX> __device__ __forceinline__ float rnd_act(float v)
{
    if constexpr (sizeof(TX) == 2) return (float)(TX)v;
    else return v;
}
// six consecutive channels starting at element index idx (idx % 2 == 0)
template <typename TX> __device__ __forceinline__ void ld_act6(const void *base, size_t idx, float (&v)[6])
{
    if constexpr (sizeof(TX) == 4) {
        const f32x2 *p = (const f32x2 *)((const float *)base + idx);
        const f32x2 a = p[0], c = p[1], d = p[2];
        v[0] = a[0]; v[1] = a[1]; v[2] = c[0]; v[3] = c[1]; v[4] = d[0]; v[5] = d[1];
    } else {
        const unsigned *p = (const unsigned *)((const unsigned short *)base + idx);
        const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
        v[0] = (float)__builtin_bit_cast(TX, (unsigned short)(w0 & 0xFFFFu)); v[1] = (float)__builtin_bit_cast(TX, (unsigned short)(w0 >> 16));
        v[2] = (float)__builtin_bit_cast(TX, (unsigned short)(w1 & 0xFFFFu)); v[3] = (float)__builtin_bit_cast(TX, (unsigned short)(w1 >> 16));
        v[4] = (float)__builtin_bit_cast(TX, (unsigned short)(w2 & 0xFFFFu)); v[5] = (float)__builtin_bit_cast(TX, (unsigned short)(w2 >> 16));
    }
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <typename T> __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mfma16<__bf16>(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mfma16<_Float16>(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

#define RP_COLS 16          // elements per block of reduce_partials_kernel
// ------------------------------------------------------------------------------------ partial sums
// Weight gradients are accumulated per block and written as one row of a [blocks][count] partial-sum matrix;
// reduce_partials_kernel adds the rows in a fixed order (deterministic, and no same-address atomics: a few
// thousand fp32 atomics per address cost ~0.4 ms per launch on MI355X).
// One launch reduces up to RP_MAX_JOBS partial-sum matrices (the head and the six dilated layers; the three separable
// layers): ten separate launches of ~6 us each, serialised behind their producers, cost 65 us of the 1.57 ms bf16 step.
#define RP_MAX_JOBS 8
struct rp_job {
    const float *part;
    float *out0, *out1, *out2;
    int nblocks, count, n0, n1, block0;                        // block0: first block of this job in the batched grid
};
struct rp_batch { rp_job job[RP_MAX_JOBS]; int njobs; };

// One block's share of a job: RP_COLS consecutive elements x (256 / RP_COLS) row groups.  Loads in flight per thread: 32 while the
// matrix has that many rows per group left, then 8, then 1 -- the additions happen in the order of the plain 8-wide loop either way
// (acc[u] takes rows ty + G u, + 8 G, + 16 G, ... one after the other), so the stand-alone kernel and the in-kernel tail below give
// the same bits.  s: 256 floats of LDS.
__device__ __forceinline__ void rp_reduce_group(const rp_job &J, int blk, float *s)
{
    const float *__restrict__ part = J.part;
    const int nblocks = J.nblocks, count = J.count, n0 = J.n0, n1 = J.n1;
    constexpr int G = 256 / RP_COLS;
    const int tx = threadIdx.x % RP_COLS, ty = threadIdx.x / RP_COLS;
    const int e = blk * RP_COLS + tx;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (e < count) {
        int b = ty;
        for (; b + 31 * G < nblocks; b += 32 * G) {
            float v[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int u = 0; u < 8; ++u) v[k][u] = part[(size_t)(b + G * (8 * k + u)) * count + e];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] += v[k][u];
        }
        for (; b + 7 * G < nblocks; b += 8 * G) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += part[(size_t)(b + G * u) * count + e];
        }
        for (; b < nblocks; b += G) acc[0] += part[(size_t)b * count + e];
    }
    s[ty * RP_COLS + tx] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    __syncthreads();
    if (ty == 0 && e < count) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) v += s[g * RP_COLS + tx];           // fixed order: deterministic
        if (e < n0) J.out0[e] = v;
        else if (e < n0 + n1) J.out1[e - n0] = v;
        else J.out2[e - n0 - n1] = v;
    }
    __syncthreads();
}

// bf16 train step: a weight-gradient kernel ends by totalling the partial rows of the producer IN FRONT of it (complete: stream
// order) -- the rows are microseconds old and still in the Infinity Cache, every block takes one or two column groups with
// 32 loads in flight, and the two stand-alone reduction launches of a pass (15.8 us each: 92 MB read back from memory) disappear.
// part == nullptr: nothing to do.  s: 256 floats of LDS that nobody else touches any more (the caller has passed a barrier).
__device__ __forceinline__ void rp_reduce_tail(const rp_job &J, float *s)
{
    if (J.part == nullptr) return;                                               // kernel-uniform
    const int ngroups = (J.count + RP_COLS - 1) / RP_COLS;
    for (int g = (int)blockIdx.x; g < ngroups; g += (int)gridDim.x) rp_reduce_group(J, g, s);
}

// Sum the four waves' 224 x 32 accumulator sets and write this block's row of the partial-sum matrix
// ([216*24 kernel gradient | 24 bias gradient]).  Waves take turns adding into one lane-linear LDS image
// (ds_read/write_b128, conflict-free): LDS float atomics cost ~3 cycles per LANE on gfx950 and made this epilogue
// the longest phase of the kernel.
// MT: accumulator tiles per wave, starting at M tile mt0 (a block of 4 x (14 / MT) waves: `ks` = the wave's k-step class, the order of the sum)
template <int MT = 14>
__device__ __forceinline__ void wgrad_block_reduce(const f32x4 (&acc)[MT][2], float *__restrict__ red /* 28 KiB */,
                                                   float *__restrict__ prow, int lane, int ks, int mt0 = 0)
{
    f32x4 *img = (f32x4 *)red;                         // [(mt, nt)][lane] x 4 floats (r)
    __syncthreads();                                   // tile buffers are free now
    for (int ph = 0; ph < 4; ++ph) {
        if (ks == ph) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    f32x4 v = acc[mt][nt];
                    if (ph > 0) v += img[((mt0 + mt) * 2 + nt) * 64 + lane];
                    img[((mt0 + mt) * 2 + nt) * 64 + lane] = v;
                }
        }
        __syncthreads();
    }
    // D layout: col = lane & 15 (co), row = 4 * (lane >> 4) + r (rho within the M tile)
    for (int t = threadIdx.x; t < 217 * UBD_C; t += blockDim.x) {
        const int row = t / UBD_C, col = t - row * UBD_C;
        const int mt = row >> 4, rr = row & 15, nt = col >> 4;
        const int ln = 16 * (rr >> 2) + (col & 15);
        prow[t] = red[(((mt * 2 + nt) * 64 + ln) << 2) + (rr & 3)];
    }
}

// ------------------------------------------------------------------------------------ head weight gradient
// dhk[c][k] = sum_p a9[p][c] dl[p][k]; dhb[k] = sum_p dl[p][k]  (row 24 of the A operand is all ones); k_out > 1.
// Tiles of 64 pixels are staged through LDS with contiguous 16-byte loads (activations widened to fp32, a ones column
// appended) and the MFMA operands are read back in their layout: lane (m, kq) takes A[c = m (+16)][px = 4 s + kq] and
// B[px][k = m (+16)].  Row stride 48 floats: the four pixel rows of a k-step start 16 banks apart (conflict-free).
// Wave w multiplies pixels 16 w .. 16 w + 15 of every tile.
#define HW_TILE 64
#define HW_STRIDE 48
// DXOUT (bf16 train step with classes, round 4): the head's DATA gradient G9 = (dlogits . hk^T) * (A9 > 0), rounded to TX, leaves from the same staged
// tile -- head_dx16_kernel read the 48 bytes per pixel of A9 a second time (22.5 + 23.7 us at 64 images and 8 classes).  Same expression in the
// same order as head_dx16_kernel (fmaf chain over the output channels k = 0, 1, ..): bit-identical G9.
template <typename TX, bool DXOUT = false>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const void *__restrict__ a9, const float *__restrict__ dlogits,
                                                         float *__restrict__ partials, long npix, int k_out,
                                                         const float *__restrict__ hk = nullptr, unsigned short *__restrict__ gout = nullptr)
{
    static_assert(!DXOUT || sizeof(TX) == 2, "the 16-bit gradient tensor");
    __shared__ __attribute__((aligned(16))) float s_kT[DXOUT ? (UBD_MAX_CLASSES + 1) * UBD_C : 4];   // head kernel transposed: [k][c]
    if constexpr (DXOUT)
        for (int t = threadIdx.x; t < UBD_C * k_out; t += 256) { const int c = t / k_out, k = t - c * k_out; s_kT[k * UBD_C + c] = hk[t]; }   // visible after the first barrier of the tile loop
    __shared__ __attribute__((aligned(16))) float sA[HW_TILE * HW_STRIDE];      // [px][c (24) | 1 | zeros]
    __shared__ __attribute__((aligned(16))) float sB[HW_TILE * (UBD_MAX_CLASSES + 1) + 32];   // flat copy of the tile's dlogits: [px][k_out]; columns k >= k_out
                                                                                            // of the B operand read the next pixel's values and are dropped at the end
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    for (int t = threadIdx.x; t < HW_TILE * HW_STRIDE; t += 256) {                // ones column, zero padding (written once)
        const int c = t % HW_STRIDE;
        sA[t] = c == UBD_C ? 1.f : 0.f;
    }
    for (int t = threadIdx.x; t < HW_TILE * (UBD_MAX_CLASSES + 1) + 32; t += 256) sB[t] = 0.f;
    f32x4 acc[2][2] = {};
    const long ntiles = (npix + HW_TILE - 1) / HW_TILE;
    const bool wide = k_out > 16;
    // register staging: the next tile's global loads are in flight while the current tile is multiplied
    constexpr int CPP = sizeof(TX) == 4 ? 6 : 3, EPC = 16 / sizeof(TX);          // 16-byte chunks per pixel, elements per chunk
    constexpr int AREGS = (HW_TILE * CPP + 255) / 256;                            // 2 (fp32) / 1 (16-bit)
    constexpr int BREGS = (HW_TILE * (UBD_MAX_CLASSES + 1) + 255) / 256;          // 8
    u32x4 ra[AREGS];
    float rb[BREGS];
    auto fetch = [&](long tile) {
        const long p0 = tile * HW_TILE;
#pragma unroll
        for (int r = 0; r < AREGS; ++r) {
            const int ch = r * 256 + threadIdx.x;
            const int px = ch / CPP;
            const u32x4 z = {0u, 0u, 0u, 0u};
            ra[r] = (ch < HW_TILE * CPP && p0 + px < npix) ? ((const u32x4 *)a9)[p0 * CPP + ch] : z;
        }
#pragma unroll
        for (int r = 0; r < BREGS; ++r) {
            const int e = r * 256 + threadIdx.x;
            rb[r] = (e < HW_TILE * k_out && p0 * k_out + e < npix * k_out) ? dlogits[p0 * k_out + e] : 0.f;
        }
    };
    long tile = blockIdx.x;
    if (tile < ntiles) fetch(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        const long p0 = tile * HW_TILE;
        __syncthreads();                                                          // previous tile's operands consumed
#pragma unroll
        for (int r = 0; r < AREGS; ++r) {
            const int ch = r * 256 + threadIdx.x;
            if (ch < HW_TILE * CPP) {
                const int px = ch / CPP, part = ch - px * CPP;
                float *dst = sA + px * HW_STRIDE + part * EPC;
                if constexpr (sizeof(TX) == 4) {
                    *(f32x4 *)dst = __builtin_bit_cast(f32x4, ra[r]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        dst[2 * e] = (float)__builtin_bit_cast(TX, (unsigned short)(ra[r][e] & 0xFFFFu));
                        dst[2 * e + 1] = (float)__builtin_bit_cast(TX, (unsigned short)(ra[r][e] >> 16));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < BREGS; ++r) {
            const int e = r * 256 + threadIdx.x;
            if (e < HW_TILE * k_out) sB[e] = rb[r];
        }
        if (p0 + HW_TILE > npix)                                                  // ragged last tile: no ones beyond the data
            for (int px = threadIdx.x; px < HW_TILE; px += 256) sA[px * HW_STRIDE + UBD_C] = (p0 + px < npix) ? 1.f : 0.f;
        __syncthreads();
        if (tile + gridDim.x < ntiles) fetch(tile + gridDim.x);
        if constexpr (DXOUT) {
            // one 16-byte chunk (8 channels of a pixel) per thread: 192 of the 256 threads; the pixel's d logits come from sB (broadcast reads),
            // the weights of the eight channels as two ds_read_b128 per output channel, the ReLU mask from the staged activation (fp32 copy: > 0)
            if (threadIdx.x < HW_TILE * 3) {
                const int px = (int)threadIdx.x / 3, c8 = (int)threadIdx.x - 3 * px;
                float g8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                for (int k = 0; k < k_out; ++k) {
                    const float dl = sB[px * k_out + k];
                    const f32x4 w0 = *(const f32x4 *)&s_kT[k * UBD_C + c8 * 8], w1 = *(const f32x4 *)&s_kT[k * UBD_C + c8 * 8 + 4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { g8[e] = fmaf(dl, w0[e], g8[e]); g8[4 + e] = fmaf(dl, w1[e], g8[4 + e]); }
                }
                const f32x4 a0 = *(const f32x4 *)&sA[px * HW_STRIDE + c8 * 8], a1 = *(const f32x4 *)&sA[px * HW_STRIDE + c8 * 8 + 4];
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float alo = e < 2 ? a0[2 * e] : a1[2 * e - 4], ahi = e < 2 ? a0[2 * e + 1] : a1[2 * e - 3];
                    const unsigned lo = alo > 0.f ? (unsigned)__builtin_bit_cast(unsigned short, (TX)g8[2 * e]) : 0u;
                    const unsigned hi = ahi > 0.f ? (unsigned)__builtin_bit_cast(unsigned short, (TX)g8[2 * e + 1]) : 0u;
                    o[e] = lo | (hi << 16);
                }
                if (p0 + px < npix) ((u32x4 *)gout)[(p0 + px) * 3 + c8] = o;
            }
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int px = 16 * wid + 4 * s4 + kq;
            const float a0 = sA[px * HW_STRIDE + m], a1 = sA[px * HW_STRIDE + 16 + m];
            const float b0 = sB[px * k_out + m];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            if (wide) {
                const float b1 = sB[px * k_out + 16 + m];
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    // D: col = lane&15 (k index), row = 4*(lane>>4) + r (channel index / ones row).  Block reduction in LDS first.
    __syncthreads();
    float *red = sA;                                                              // 32 x 32 floats
    for (int t = threadIdx.x; t < 32 * 32; t += blockDim.x) red[t] = 0.f;
    __syncthreads();
    // the four waves add their tiles one after the other (every (row, column) belongs to one lane per wave): a fixed order, so the
    // head gradients of a multi-class model repeat bit for bit like everything else (round 4; LDS float atomics added them in
    // whatever order the waves arrived)
    for (int ph = 0; ph < 4; ++ph) {
        if (wid == ph) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[(16 * mt + 4 * kq + r) * 32 + m + 16 * nt] += acc[mt][nt][r];
        }
        __syncthreads();
    }
    // one partial row [c (24) | ones][k_out] per block, summed by reduce_partials_kernel (a thousand blocks adding into the
    // same 25 k_out addresses would serialise for tens of microseconds)
    for (int t = threadIdx.x; t < 25 * 32; t += blockDim.x) {
        const int row = t >> 5, col = t & 31;
        if (col < k_out) partials[(size_t)blockIdx.x * (25 * k_out) + row * k_out + col] = red[t];
    }
}

// k_out == 1 (detection only, the benchmark configuration): dhk[c] = sum_p a9[p][c] dl[p], dhb = sum_p dl[p] is a
// plain streaming reduction: one pixel per lane per step (the 24 channels are 96 / 48 contiguous bytes), 25 fp32
// accumulators per lane, butterfly reduction per wave, one partial row per block (summed by reduce_partials_kernel).
template <typename TX>
__global__ __launch_bounds__(256) void head_wgrad1_kernel(const void *__restrict__ a9, const float *__restrict__ dlogits,
                                                          float *__restrict__ partials, long npix)
{
    float acc[UBD_C + 1];
#pragma unroll
    for (int c = 0; c <= UBD_C; ++c) acc[c] = 0.f;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const float dl = dlogits[p];
        float av[UBD_C];
#pragma unroll
        for (int c6 = 0; c6 < 4; ++c6) {
            float t6[6];
            ld_act6<TX>(a9, (size_t)p * UBD_C + 6 * c6, t6);
#pragma unroll
            for (int e = 0; e < 6; ++e) av[6 * c6 + e] = t6[e];
        }
#pragma unroll
        for (int c = 0; c < UBD_C; ++c) acc[c] = fmaf(av[c], dl, acc[c]);
        acc[UBD_C] += dl;
    }
    __shared__ float s_red[4][UBD_C + 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c <= UBD_C; ++c) {
        float v = acc[c];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) s_red[wid][c] = v;
    }
    __syncthreads();
    if (threadIdx.x <= UBD_C)
        partials[(size_t)blockIdx.x * (UBD_C + 1) + threadIdx.x] = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}


// Host side of the batched reduction: every producer takes its own partial-sum matrix out of the workspace region and
// queues a job; rp_flush launches the jobs queued so far (after the dilated loop: those gradients feed the overlapped
// all-reduce; at the end of the pass).
struct rp_queue {
    rp_batch b;
    int nblocks;
    float *base;
    size_t used, cap;                                          // floats
};
void rp_init(rp_queue *q, float *base, size_t cap_floats);
// bf16 pass: the job queued last is handed to the NEXT producer kernel, which totals it at its end (rp_reduce_tail) -- rp_take_prev
// removes it from the batch (or returns an empty job); whatever is still queued when rp_flush is called goes to the stand-alone kernel
rp_job rp_take_prev(rp_queue *q);
int rp_flush(rp_queue *q, hipStream_t st);
// a [rows][count] matrix for the next producer, reduced into out0[n0] | out1[n1] | out2[rest]
float *rp_add(rp_queue *q, int rows, int count, float *out0, int n0, float *out1, int n1, float *out2, hipStream_t st);

// ------------------------------------------------------------------------------------ host
// Workspace of a train step: forward layout (all activations kept; fp32 or 16-bit), then backward fragments,
// logits, dlogits, fp32 gradient ping-pong buffers, loss scratch, partial-sum matrix.
struct train_layout {
    ubd_fwd_layout fwd;            // dtype == UBD_F32
    ubd_fwd16_layout fwd16;        // 16-bit activations
    size_t off_bfrag, off_logits, off_dlogits, off_gq[2], off_ddw3, off_gb[2], off_loss, off_partials, partials_floats, total;
};

template <int V> using int_c = std::integral_constant<int, V>;      // a template argument chosen at run time: f(int_c<V>()) for a generic lambda f

// Weight gradient of the head.  DXOUT (bf16 train step with classes): the head's data gradient as well, from the same pass over A9 --
// g = (dlogits . hk^T) * (A9 > 0) in bf16 (head_wgrad_kernel<TX, true>)
template <typename TX, bool DXOUT = false>
static int launch_head_wgrad(const ubd_handle *h, const void *a9, const float *dlogits, float *grads, rp_queue *rq, long npix,
                              hipStream_t st, const float *hk = nullptr, unsigned short *g = nullptr)
{
    if (!DXOUT && h->k_out == 1) {
        const int g1 = (int)std::min<long>((npix + 255) / 256, h->num_cus * 4);
        float *partials = rp_add(rq, g1, UBD_C + 1, grads + h->off_head_k, UBD_C, grads + h->off_head_b, 1, nullptr, st);
        if (!partials) return -1;
        hipLaunchKernelGGL((head_wgrad1_kernel<TX>), dim3(g1), dim3(256), 0, st, a9, dlogits, partials, npix);
        return 0;
    }
    const int g2 = (int)std::min<long>((npix + HW_TILE - 1) / HW_TILE, h->num_cus * 4);
    float *partials = rp_add(rq, g2, (UBD_C + 1) * h->k_out, grads + h->off_head_k, UBD_C * h->k_out, grads + h->off_head_b, h->k_out, nullptr, st);
    if (!partials) return -1;
    hipLaunchKernelGGL((head_wgrad_kernel<TX, DXOUT>), dim3(g2), dim3(256), 0, st, a9, dlogits, partials, npix, h->k_out, hk, g);
    return 0;
}

// L1 reads the images, which have 1 or 3 channels: f gets the count as an int_c, so that a caller writes its launch once
template <typename F> static int with_c_in(const ubd_handle *h, F f) { return h->cfg.c_in == 1 ? f(int_c<1>()) : f(int_c<3>()); }

// what L1 does to a raw pixel before the first convolution: (x - sub) / div; u8: the images are uint8
struct input_affine_t { float sub, div; int u8; };
static input_affine_t input_affine(int preprocessing, int in_dtype)
{
    const bool mobilenet = preprocessing == UBD_PRE_MOBILENET;
    return {mobilenet ? 127.5f : 0.f, mobilenet ? 127.5f : 1.f, in_dtype == UBD_IN_U8};
}

// arguments of the bf16 step's one-launch prologue (bwd16.hip); fill_pack_args fills the packers' part, which the fp32 pass uses too
struct train_prologue_args {
    pack_args pa;
    pack_bwd_args pb;
    pack_sep16_args ps;
    size_t off0, layer_stride, n_params, loss_zero_words;
    float *wfrag32, *bfrag, *grads;
    unsigned *wfrag16, *frag16t, *loss_zero;
};

// the part of the packers' arguments that comes from the handle (parameter offsets and counts); the buffers are the caller's
static train_prologue_args fill_pack_args(const ubd_handle *h)
{
    train_prologue_args a = {};
    for (int s = 0; s < 3; ++s) { a.pa.off_sep_dw[s] = h->off_sep_dw[s]; a.pa.off_sep_pw[s] = h->off_sep_pw[s]; a.pb.off_sep_pw[s] = h->off_sep_pw[s]; }
    for (int k = 0; k < UBD_NUM_DIL; ++k) { a.pa.off_dil_k[k] = h->off_dil_k[k]; a.pb.off_dil_k[k] = h->off_dil_k[k]; }
    a.pa.c_in = a.pb.c_in = h->cfg.c_in;
    a.ps = ubd_pack_sep16_args(h);
    a.off0 = h->off_dil_k[0]; a.layer_stride = h->off_dil_k[1] - h->off_dil_k[0];
    a.n_params = h->n_params;
    return a;
}

// end of either pass: the partial sums still queued, launch errors, the rest of the overlapped all-reduce
static int finish_step(ubd_handle *h, rp_queue *rq, float *grads, hipStream_t st)
{
    rp_flush(rq, st);
    UBD_CHECK_HIP(hipGetLastError());
    return ubd_comm_fused(h) ? ubd_comm_finish(h, grads, st) : 0;
}

// A train step's backward pass.  Its data: the step's arguments, the loss gradient, the carved workspace, and what the forward pass
// kept -- a1, a2 at half resolution and acts[0..6] = the outputs of L3, L4..L9 at quarter resolution, in the handle's dtype, and its
// fp32 fragments wfrag (depthwise / pointwise per-lane weights).  One of backward_f32<TX> (bwd32.hip) / backward_bf16 (bwd16.hip) runs it.
struct bwd_pass {
    ubd_handle *h; const float *params; const void *images; int in_dtype, preprocessing, n, H, W;
    float *dlogits, *grads; char *ws; const train_layout &T; hipStream_t st;
    const void *a1, *a2, *acts[7]; const float *wfrag;      // filled in after the forward pass
    template <typename TX> int backward_f32();
    template <typename TX> int sep_backward_f32(const float *G3, rp_queue *rq);
    void prologue_bf16();      // in front of the forward pass
    int backward_bf16();
};

// backward.hip: the workspace layout of a step, and its two halves around the loss (forward with kept activations; backward pass)
void ubd_train_layout_compute(const ubd_handle *h, int n, int H, int W, train_layout *T);
int ubd_train_forward(bwd_pass &p, float *logits);
int ubd_train_backward(bwd_pass &p);
