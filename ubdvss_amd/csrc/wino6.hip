// Dense dilated 3x3 convolution 24 -> 24, fp32 in / fp32 out, as Winograd F(2x2, 3x3) on the dilation sub-grids with the 16
// transform-domain GEMMs computed as SPLIT PRODUCTS on the 16-bit MFMAs (fp32 accumulate): by default two fp16 pieces per value
// under power-of-two scales on v_mfma_f32_16x16x32_f16, three MFMAs per product; with UBD_DILCONV=split3 three bf16 pieces on
// v_mfma_f32_16x16x32_bf16, six MFMAs per product (the form of rounds 6..14, the reference side of tests/test_gpu_wino6_f16.py).
//
// Reference semantics: conv_bn(dilation_rate=d) (semantic_segmentation/net.py:298-304): 'same' zero padding d per side,
// cross-correlation, + bias + ReLU (and, for the last layer of an inference pass with one output channel, the 1x1 head of
// net.py:308-311 in the epilogue).  Same tiling, addressing and transforms as wino.hip (the fp32-MFMA form, kept for the data
// gradient and as the reference side of the bit-level tests); what changes is the arithmetic of the products.
//
// Why 16-bit MFMAs: the fp32 MFMA (v_mfma_f32_16x16x4_f32) runs at the fp32 VECTOR rate -- 32 cycles of its SIMD per
// instruction, 192 per group of 16 tiles -- and the fp32 vector work of the transforms does not overlap with it (times add:
// DESIGN.md 5.1a), which left the layer at 36 us for 32 x 128 x 128 maps.  A 16-bit MFMA of the same shape class takes 16 cycles
// for EIGHT times the K, holds the vector issue port for 8 of them only, and fp32 vector instructions run beside it.  K = 24
// input channels fit ONE K = 32 step, so a (transform point, N tile) costs one MFMA per piece product.
//
// Three bf16 pieces (F16 = false): every fp32 value v is the EXACT sum of three bf16 values obtained by truncation,
//     v = v1 + v2 + v3,   v1 = hi16(v),  v2 = hi16(v - v1),  v3 = hi16(v - v1 - v2)       (8 + 8 + 8 = 24 significand bits),
// and the six piece products with i + j <= 4 are kept (the three dropped ones are <= 2^-24 of the product): 192 MFMAs per group,
// 96 KiB of weight pieces, 5.5 vector instructions per sample value for the split (v_and / v_sub / v_perm).  bf16 has fp32's
// exponent range, so no scale is needed.  The layer was bound by the SIMD's shared issue port (matrix pipe busy 44 % of the
// launch, vector ALU 66 %, either 94 %: profiles/r06_experiment_notes.txt A.4), so instructions had to go.
//
// Two fp16 pieces (F16 = true, the default): fp16 carries 11 significand bits, two pieces 22,
//     h1 = f16(x),  h2 = f16(x - h1)   both rounded to NEAREST (truncation costs 4x the error: tools/sim_f16_split.py),
// and THREE piece products are kept, chained from the smallest to the largest so that the big term is rounded once:
// h2 g1, then h1 g2, then h1 g1 (the dropped h2 g2 is <= 2^-22 of the product's bound).  96 MFMAs per group, 64 KiB of weight
// pieces (4 ds_read_b128 per point instead of 6), 2 vector instructions per value for the split (per pair of values
// v_cvt_pk_f16_f32, 2 x v_fma_mix_f32 for x - h1 with h1 read as fp16, v_cvt_pk_f16_f32; with UBD_WINO6_SPLIT=cvt the 3 per
// value of round 15: v_cvt_pk_f16_f32, v_cvt_f32_f16, v_sub -- the same bits) plus one for the scale.  fp16's narrow exponent
// range is handled EXACTLY by power-of-two scales (split2h.h):
//   * weights: one scale t per layer, max |U| t in [2^12, 2^13), applied at pack time; 1 / t rides behind the fragments;
//   * samples: one scale s per TILE and TRANSFORM ROW a, from the largest |T| of the row's 4 x 24 values T = (B^T D)[a] (the four
//     lanes i, i + 16, i + 32, i + 48 hold a tile's channel quarters: v_max3 in the lane, two v_permlane swaps across);
//     |V| <= 2 max |T| and max |T| s in [2^13, 2^14), so |V s| < 2^15.  Per row, not per tile, because only three of a tile's
//     four sample rows are live at a time, and a row's own scale is the tighter one.  The scale never looks at another tile, so
//     results do not depend on which tiles share a wave (tests/test_gpu_wino6_layout.py: bit-identity of the groupings);
//   * a lane's four accumulators are four output channels of the lane's own tile, so unscaling is lane-local: the output
//     transform along a adds Z / (s t) into Y with one fma per term, which replaces the add (the product is exact).
// Scales are powers of two and commute with every rounding: f(2^k x) = 2^k f(x) stays bit-exact, an all-zero kernel gives
// relu(bias) exactly, and a small image beside a large one, or a small region of a map, keeps its own 22 bits.
// Measured (profiles/r15_wino6_f16_notes.txt): error against fp64 <= 2.0e-7 of max |y| per layer (three pieces 1.8e-7, fp32
// MFMA 2.5e-7).
#include "common.h"
#include "split3.h"
#include "split2h.h"

// U fragments of one layer, three-piece form: [xi = a*4+b (16)][nt (2)][piece (3)][lane (64)] x 4 dwords (8 bf16 k-slots of the lane's k-group)
//   lane = (m = lane & 15 : output channel co = m + 16 nt, zero rows for co >= 24;  q = lane >> 4 : k-group)
//   k-slot e of group q holds input channel ci = e < 4 ? 4q + e : 16 + 2q + (e - 4) for e < 6, zero for e = 6, 7
//   (the same channel-to-lane map as the sample registers of the kernel: the input transform stays lane-local)
struct wino6_pack_args { size_t off_dil_k[UBD_NUM_DIL]; };

__global__ void pack_wino6_kernel(const float *__restrict__ params, unsigned *__restrict__ out, wino6_pack_args a)
{
    const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
    const int total = UBD_NUM_DIL * 16 * 2 * 64;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int lane = idx & 63, nt = (idx >> 6) & 1, xi = (idx >> 7) & 15, L = idx >> 11;
        const int q = lane >> 4, co = (lane & 15) + 16 * nt;
        const int ta = xi >> 2, tb = xi & 3;
        unsigned p[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        if (co < UBD_C) {
            const float *wk = params + a.off_dil_k[L];
            for (int e = 0; e < 6; ++e) {
                const int ci = e < 4 ? 4 * q + e : 16 + 2 * q + (e - 4);
                float v = 0.f;
                for (int ky = 0; ky < 3; ++ky)
                    for (int kx = 0; kx < 3; ++kx)
                        v += G[ta][ky] * G[tb][kx] * wk[((ky * 3 + kx) * UBD_C + ci) * UBD_C + co];
                unsigned b[3];
                split3_bits(v, b);                             // exact three-way truncation split
                const int sh = (e & 1) ? 0 : 16;              // even slot: low half of the dword
                p[0][e >> 1] |= b[0] >> sh;
                p[1][e >> 1] |= b[1] >> sh;
                p[2][e >> 1] |= b[2] >> sh;
            }
        }
        unsigned *o = out + ((size_t)(idx >> 6) * 3 * 64 + lane) * 4;      // idx >> 6 = (L * 16 + xi) * 2 + nt
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
            *(u32x4 *)(o + pc * 64 * 4) = (u32x4){p[pc][0], p[pc][1], p[pc][2], p[pc][3]};
    }
}

// The fp16 form: U fragments [xi (16)][nt (2)][piece (2)][lane (64)] x 4 dwords (8 fp16 k-slots, the lane and slot maps above) of
// U t, where t is ONE power of two per layer with max |U| t in [2^12, 2^13) (split2h.h: the small piece of the largest weights
// then sits 11 binades above fp16's subnormals; t = 1 for an all-zero kernel), and 1 / t behind the fragments, at dword
// UBD_WINO6_FRAG_U32 of the layer's slot.  Four blocks per layer; each finds the layer's max |U| itself (9216 values, nine per thread).
#define W6_PACK_BLOCKS 4
__device__ __forceinline__ float wino6_u(const float *wk, int ta, int tb, int ci, int co)
{
    const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
    float v = 0.f;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx)
            v += G[ta][ky] * G[tb][kx] * wk[((ky * 3 + kx) * UBD_C + ci) * UBD_C + co];
    return v;
}
__global__ __launch_bounds__(1024) void pack_wino6h_kernel(const float *__restrict__ params, unsigned *__restrict__ out, wino6_pack_args a)
{
    __shared__ unsigned s_max;
    const int L = blockIdx.x / W6_PACK_BLOCKS, part = blockIdx.x % W6_PACK_BLOCKS;
    const float *wk = params + a.off_dil_k[L];
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    unsigned mx = 0u;
    for (int j = threadIdx.x; j < 16 * UBD_C * UBD_C; j += blockDim.x) {
        const int co = j % UBD_C, ci = (j / UBD_C) % UBD_C, xi = j / (UBD_C * UBD_C);
        const unsigned b = split2h_bits(wino6_u(wk, xi >> 2, xi & 3, ci, co)) & 0x7fffffffu;
        mx = b > mx ? b : mx;
    }
    atomicMax(&s_max, mx);                                 // LDS: non-negative floats order as their bit patterns
    __syncthreads();
    unsigned t_bits, inv_bits;
    split2h_scale(s_max, SPLIT2H_WEIGHT_TOP, SPLIT2H_WEIGHT_LO, t_bits, inv_bits);
    const float t = split2h_float(t_bits);
    unsigned *slot = out + (size_t)L * UBD_WINO6_SLOT_U32;
    if (part == 0 && threadIdx.x == 0) slot[UBD_WINO6_FRAG_U32] = inv_bits;
    const int per_block = 16 * 2 * 64 / W6_PACK_BLOCKS;
    for (int k = threadIdx.x; k < per_block; k += blockDim.x) {
        const int idx = part * per_block + k;              // (xi * 2 + nt) * 64 + lane
        const int lane = idx & 63, nt = (idx >> 6) & 1, xi = idx >> 7;
        const int q = lane >> 4, co = (lane & 15) + 16 * nt;
        unsigned p[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (co < UBD_C) {
            for (int e = 0; e < 6; ++e) {
                const int ci = e < 4 ? 4 * q + e : 16 + 2 * q + (e - 4);
                float g1, g2;
                split2h_pieces(wino6_u(wk, xi >> 2, xi & 3, ci, co) * t, g1, g2);
                const int sh = (e & 1) ? 16 : 0;          // even slot: low half of the dword
                p[0][e >> 1] |= split2h_f16_bits(g1) << sh;
                p[1][e >> 1] |= split2h_f16_bits(g2) << sh;
            }
        }
        unsigned *o = slot + ((size_t)(idx >> 6) * 2 * 64 + lane) * 4;
#pragma unroll
        for (int pc = 0; pc < 2; ++pc)
            *(u32x4 *)(o + pc * 64 * 4) = (u32x4){p[pc][0], p[pc][1], p[pc][2], p[pc][3]};
    }
}

void ubd_launch_pack_wino6(const ubd_handle *h, const float *params, unsigned *out, hipStream_t st)
{
    wino6_pack_args a;
    for (int k = 0; k < UBD_NUM_DIL; ++k) a.off_dil_k[k] = h->off_dil_k[k];
    if (h->wino6_split3) hipLaunchKernelGGL(pack_wino6_kernel, dim3(48), dim3(256), 0, st, params, out, a);
    else hipLaunchKernelGGL(pack_wino6h_kernel, dim3(UBD_NUM_DIL * W6_PACK_BLOCKS), dim3(1024), 0, st, params, out, a);
}

// All arithmetic below is plain C++ on vector types (no inline asm):
//   * hipcc's scheduler and hazard recogniser see every instruction -- an asm v_add_f32 that reads an MFMA destination gets none of
//     the wait states the read needs (observed with the first version of this kernel: register 0 of the result correct, 1..3 stale);
//   * the two-component adds compile to v_pk_add_f32.  Measured on gfx950 (tools/ubench/valu_ops.hip): a wave issues a simple vector
//     instruction every ~2.9 ns when it runs alone and the SIMD sustains one per ~1.1 ns from 2+ waves, while v_pk_add_f32 takes
//     ~2.25 ns per instruction at ANY occupancy.  At the two waves per SIMD this kernel's 250 registers allow, the waves are bound by
//     their own issue interval, so halving the number of add instructions halves their time (the fp32-MFMA kernel next door avoided the
//     packed form for the opposite reason: beside fp32 MFMAs it sits in the MFMA's shadow at one wave per SIMD).
//   Other per-instruction prices that shaped the code (same file): v_perm_b32 / v_cvt_pk_bf16_f32 / v_max_f32 / v_add3_u32 / any
//   instruction with an SGPR source ~1.95 ns, v_and_b32 with a literal 1.05 ns, s_nop and scalar ALU ~1.9 ns of the wave's time.
// resid / pack_hi / pack6 / mfma16: split3.h

// diagnostic build only (stamps.h): eight slots per wave, no tile index (tools/stamps_wino6.py)
#define WSTAMP(cond, k) UBD_STAMP(cond, ((size_t)blockIdx.x * W6_WAVES + wave_in_block) * 8 + (k))

#ifndef W6_WAVES
#define W6_WAVES 8
#endif
struct w6samples {
    f32x4 v4[4][4];
    f32x2 v2[4][4];
};
// Column layouts of the activation rows.  P_p (p a power of two) keeps pixel x of a row at position
//     (x mod p) floor(W / p) + min(x mod p, W mod p) + floor(x / p):
// the row's pixels phase by phase, an exact permutation (P_1 = natural order).  A layer of dilation d that reads P_2d groups the 16
// tiles of one sub-grid phase (phase grouping): each column-b sample load then covers ONE run of 16 pixels, where the natural grouping
// spreads it over 16 pixels 2 apart at d = 1 (~20 cache lines per instruction instead of ~12; d >= 4 already reads runs of 4 or more).
// Stores go to any P_p; the Winograd arithmetic of a tile does not depend on which lane holds it, so the results are bit-identical.
// launch geometry (host): everything the group decode needs, so that the loop holds no integer division
struct w6geom {
    int n, h, w, d, log2d;
    unsigned in_bytes;
    unsigned groups_x, half_rows, total;
    unsigned magic_gx, magic_hr;      // floor(v / groups_x) = umulhi(v, magic_gx) for v < total (ubd_tile_decoder's rule)
    int wpb;                          // waves per block that take groups (1..8): small launches spread over more CUs (all 8 waves copy the weights)
    int phase;                        // 1: input in layout P_2d and every group confined to one sub-grid phase; 0: natural input and grouping
    int l2po;                         // log2 of the output layout's period (0: natural)
};
// addresses of one group: wave-uniform row terms (scalar registers; they ride in the buffer instructions' soffset, which IS part of
// the hardware range check: tools/ubench/buf_soffset.hip) and per-lane column terms.  An invalid row or column is 2^30 (host: tensor
// bytes <= 2^30), so any sum with an invalid term is out of range: loads return the zero padding, stores are dropped.
struct w6addr {
    unsigned row[4];      // byte offset of pixel (sample row a, x = 0)
    unsigned lrow[2];     // EPI 2: byte offset of logit (output row rr, x = 0)
    unsigned c4[4];       // column b: this lane's 16-byte chunk (channels 4q ..)
    unsigned c2[4];       // column b: this lane's 8-byte chunk (channels 16 + 2q, 17 + 2q)
    unsigned oc[2];       // output column c (pixel of sample column 1 + c) in the output layout: this lane's 16-byte chunk
};

// EPI 0: y = relu(conv + bias);  EPI 2: logits = head(relu(conv + bias)) (one output channel; y is never written)
// LAY: false = natural input and output (layout terms compiled out), true = the layouts of G.phase / G.l2po
// F16: true = two fp16 pieces under per-row scales, 3 MFMAs per product (the default); false = three bf16 pieces, 6 MFMAs (UBD_DILCONV=split3)
// MIX (F16 only): true = the residual x - h1 of the sample split by v_fma_mix_f32 (split2h_6m: 4 instructions per pair of values, the
//      default); false = by two conversions and a subtraction (split2h_6: 6 per pair, UBD_WINO6_SPLIT=cvt -- the form of round 15, the
//      reference side of tests/test_gpu_wino6_mix.py).  The same bits either way.
#ifndef W6_MIX_FILL
#define W6_MIX_FILL 2      // vector instructions placed behind each MFMA of a point in the MIX form: the next point's split is 12 for 6 MFMAs
#endif
template <int EPI, bool LAY, bool F16 = true, bool MIX = F16>
__global__ __launch_bounds__(64 * W6_WAVES) void dilconv_wino6_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                                     const unsigned *__restrict__ ufrag,
                                                                     const float *__restrict__ bias, w6geom G, const float *__restrict__ head UBD_STAMP_PARAM)
{
    static_assert(F16 || !MIX, "the fma residual belongs to the fp16 form");
    constexpr int NPC = F16 ? 2 : 3;                                                 // pieces per weight
    constexpr int FRAG_U32 = F16 ? UBD_WINO6_FRAG_U32 : UBD_WINO6_FRAG3_U32;
    __shared__ __attribute__((aligned(16))) unsigned s_u[FRAG_U32];                  // 64 KiB (96 KiB for three pieces)
    const int lane = threadIdx.x & 63;
    const int i = lane & 15, q = lane >> 4;
    const int h = G.h, w = G.w, d = G.d, log2d = G.log2d, dm1 = G.d - 1;
    // Bias and head weights stay in registers for the whole kernel (8 + 8): loaded in the epilogue they cost a vmcnt(0) wait behind the
    // NEXT group's sample rows, which are in flight by then.  (An LDS table read in the epilogue was tried and looked corrupted in a few
    // per cent of the groups; the cause was the store hazard described at the stores below -- a LATER value in a store's data register --
    // not the table.  Registers are the cheaper home anyway: no reads in the epilogue.)
    const f32x4 bA = *(const f32x4 *)(bias + 4 * q);
    const f32x4 bB = q < 2 ? *(const f32x4 *)(bias + 16 + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 hA = {0.f, 0.f, 0.f, 0.f}, hB = {0.f, 0.f, 0.f, 0.f};
    float hbias = 0.f;
    if constexpr (EPI == 2) {
        hA = *(const f32x4 *)(head + 4 * q);
        if (q < 2) hB = *(const f32x4 *)(head + 16 + 4 * q);
        hbias = head[UBD_C];            // wave-uniform: one scalar load
    }
    [[maybe_unused]] float inv_t = 1.f;           // 1 / (the layer's weight scale): wave-uniform, behind the fragments (pack_wino6h_kernel)
    if constexpr (F16) inv_t = __builtin_bit_cast(float, ufrag[UBD_WINO6_FRAG_U32]);
    [[maybe_unused]] float one = 1.f;             // MIX: the factor of x 1 - h1, hidden so that the fma stays an fma (split2h_6m)
    if constexpr (MIX) asm volatile("" : "+v"(one));
    // XCD-aware split (see dilconv_f32_kernel)
    const int xcd = blockIdx.x & 7;
    const int nblk_x = (gridDim.x + 7 - xcd) >> 3;
    const int chunk = (int)((G.total + 7) >> 3);
    const int g_begin = xcd * chunk;
    const int g_end = (g_begin + chunk < (int)G.total) ? g_begin + chunk : (int)G.total;
    const int stride = nblk_x * G.wpb;

    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)x, 0, (int)G.in_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)y, 0, (int)(EPI == 2 ? G.in_bytes / UBD_C : G.in_bytes), 0x00020000);

    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int g = g_begin + (int)(blockIdx.x >> 3) * G.wpb + wave_in_block;
    const int g_last = g_end - 1;
    const unsigned BIG = 0x40000000u;
    const unsigned lane4 = 16u * q, lane2 = 64u + 8u * q;

    auto set_addr = [&](w6addr &A, int gg) {
        const unsigned rs = G.groups_x == 1u ? (unsigned)gg : __umulhi((unsigned)gg, G.magic_gx);           // gg / groups_x
        const unsigned gx = (unsigned)gg - rs * G.groups_x;
        const unsigned img = G.half_rows == 1u ? rs : __umulhi(rs, G.magic_hr);                             // rs / half_rows
        const unsigned s = rs - img * G.half_rows;
        const int y0 = (int)(((s >> log2d) << (log2d + 1)) + (s & (unsigned)dm1));
        const unsigned img_row = img * (unsigned)h;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int iy = y0 + (a - 1) * d;
            const bool ok = iy >= 0 && iy < h;
            A.row[a] = ok ? (img_row + (unsigned)iy) * (unsigned)w * (unsigned)(UBD_C * 4) : BIG;
            if (EPI == 2 && (a == 1 || a == 2)) A.lrow[a - 1] = ok ? (img_row + (unsigned)iy) * (unsigned)w * 4u : BIG;
        }
        // natural grouping: tile columns tcol = 16 gx + i;  phase grouping: gx = (block, phase ph), the 16 tiles k = 16 block + i of
        // sub-grid phase ph (tile column xj = 2d k + ph), whose column-b samples sit at positions k + const of ONE phase of P_2d
        const int ph = (int)(gx & (unsigned)dm1);
        const int tk = (int)((gx >> log2d) << 4) + i;
        const bool phase = LAY && G.phase;
        const int tcol = phase ? (tk << log2d) + ph : (int)gx * 16 + i;
        const int xj = ((tcol >> log2d) << (log2d + 1)) + (tcol & dm1);   // this lane's tile column (pixel x of output (., 0))
        const int tl = phase ? tk : xj;                                  // lane term of the input positions
        const int l2p = log2d + 1, wq = w >> l2p, wr = w & (2 * d - 1);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int ix = xj + (b - 1) * d;
            const bool ok = (unsigned)ix < (unsigned)w;
            // wave-uniform position offset: P_2d phase (ph + (b - 1) d) mod 2d, one tile on for b = 3, one back for b = 0
            const int r = ph + (b - 1) * d, rb = r & (2 * d - 1);
            const int sb = phase ? rb * wq + (rb < wr ? rb : wr) + (r >> l2p) : (b - 1) * d;
            const unsigned cb = (unsigned)(tl + sb) * (unsigned)(UBD_C * 4);
            A.c4[b] = ok ? cb + lane4 : BIG;
            A.c2[b] = ok ? cb + lane2 : BIG;
        }
        // outputs x = xj + c d, c = 0, 1, at their positions in P_(2^l2po): (x mod p) floor(w / p) + min(x mod p, w mod p) + floor(x / p)
        if constexpr (LAY) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int ox = xj + c * d;
                const int r = ox & ((1 << G.l2po) - 1);
                const int wrp = w & ((1 << G.l2po) - 1);
                const int pos = r * (w >> G.l2po) + (r < wrp ? r : wrp) + (ox >> G.l2po);
                A.oc[c] = ox < w ? (unsigned)pos * (unsigned)(UBD_C * 4) + lane4 : BIG;
            }
        } else {
            A.oc[0] = A.c4[1]; A.oc[1] = A.c4[2];
        }
    };
    auto load_row = [&](w6samples &D, const w6addr &A, int a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            D.v4[a][b] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)A.c4[b], (int)A.row[a], 0));
            D.v2[a][b] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)A.c2[b], (int)A.row[a], 0));
        }
    };

    // Sample rows are fetched just in time so that at most three of the four are live.  The first samples are requested before the
    // block copies U into LDS: their latency hides behind the copy.
    w6samples D;
    w6addr A, An;
    WSTAMP(true, 0);
    set_addr(A, g < g_last ? g : g_last);
    load_row(D, A, 0);
    load_row(D, A, 2);
    load_row(D, A, 1);
    // U (64 KiB; 96 KiB for three pieces) to LDS by LDS-DMA: 64 (96) pieces of 1 KiB, 8 (12) per wave, handed out in ROUNDS (round r,
    // wave w -> piece 8 r + w), so that the pieces of the first transform points are the first to land: pieces 0..15 (0..23) (points
    // 0..3, the first transform row) are rounds 0..1 (0..2).  The block starts computing behind THOSE (barrier A); the other six (nine)
    // rounds land under the first row of the first group and are awaited once, before point 4's weights are read (barrier B; waves
    // without a group wait there too, then leave).  The copy used to stand in front of every launch whole: ~3.5 us of a 33 us launch,
    // x 6 launches per pass.
    // (asm form: outside hipcc's bookkeeping -- its own waits for the sample rows can only over-wait, the DMAs being younger.)
    constexpr int PER_WAVE = FRAG_U32 * 4 / 1024 / W6_WAVES;                      // 8 (12)
    constexpr int EARLY_ROUNDS = 4 * 2 * NPC / W6_WAVES;                          // 2 (3): the 16 (24) pieces of points 0..3
    static_assert(PER_WAVE - EARLY_ROUNDS == (F16 ? 6 : 9), "the counted wait below is written for six (nine) late rounds");
    {
        const unsigned lds_u = ubd_lds_addr(s_u);
#pragma unroll
        for (int k = 0; k < PER_WAVE; ++k) {
            const int piece = k * W6_WAVES + wave_in_block;
            ubd_glds16_sbase((const char *)ufrag + (size_t)piece * 1024, (unsigned)lane * 16u, lds_u + (unsigned)piece * 1024u);
        }
    }
    // the sample rows (older) and this wave's early rounds have landed
    if constexpr (F16) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    __builtin_amdgcn_s_barrier();                             // A: points 0..3 of the weights are in LDS
    WSTAMP(true, 1);
    if (g >= g_end || wave_in_block >= G.wpb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // B
        return;
    }
    bool weights_pending = true;                              // wave-uniform: barrier B is still owed (first group only)
    [[maybe_unused]] int gcount = 0;
    const u32x4 *su4 = (const u32x4 *)s_u + lane;
    // Schedule of one transform point xi = 4a + b (16 per group, fully unrolled), written for the three-piece form; the fp16 form follows it with
    // 4 weight reads, one split of six values into two quads and 6 MFMAs:
    //   1. request the point's weights (6 ds_read_b128: 2 N tiles x 3 pieces);
    //   2. split the lane's six values of V[a][b] into three bf16 pieces (12 v_and + 6 v_pk_add + 9 v_perm; hides the LDS latency);
    //   3. 12 MFMAs, the two N tiles' chains alternating (no back-to-back dependent pair), with the vector work that does not
    //      feed them in the gaps: the output transform of point xi - 1 (whose accumulators are complete by now) and, at b = 3,
    //      the input transform of row a + 1.
    for (;;) {
        f32x4 Y[2][2][2];      // [output row rr][output col c][nt]
        f32x4 Z0[2], Z1[2];    // output transform along b of the current row a
        f32x4 V4[4];           // V[a][b], channels 4q .. 4q+3
        f32x2 V2[4];           //          channels 16+2q, 17+2q
        [[maybe_unused]] float inv_s[4];      // F16: 1 / (scale of transform row a x weight scale) of this lane's tile
        // V[a] = (B^T D)[a] B from the sample rows that row a needs
        auto make_v = [&](int a) {
            f32x4 T4[4];
            f32x2 T2[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (a == 0) { T4[b] = D.v4[0][b] - D.v4[2][b]; T2[b] = D.v2[0][b] - D.v2[2][b]; }
                else if (a == 1) { T4[b] = D.v4[1][b] + D.v4[2][b]; T2[b] = D.v2[1][b] + D.v2[2][b]; }
                else if (a == 2) { T4[b] = D.v4[2][b] - D.v4[1][b]; T2[b] = D.v2[2][b] - D.v2[1][b]; }
                else { T4[b] = D.v4[1][b] - D.v4[3][b]; T2[b] = D.v2[1][b] - D.v2[3][b]; }
            }
            if constexpr (F16) {
                // The scale of transform row a of this lane's TILE: from the largest |T| over the row's 4 x 24 values, which four lanes
                // hold (i, i + 16, i + 32, i + 48: the channel quarters, all k of one accumulation).  |V| <= 2 max |T|, so |V s| < 2^15.
                // A row's scale, not the tile's: the tile's fourth sample row is not here before row 3 (three of four are live), and a
                // row's own scale is the tighter one.  It depends on this tile's samples only -- never on the group -- so the result
                // does not depend on which tiles share a wave (the layouts' bit-identity), and it is a power of two.
                float mx = 0.f;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    mx = fmaxf(fmaxf(fabsf(T4[b][0]), fabsf(T4[b][1])), mx);
                    mx = fmaxf(fmaxf(fabsf(T4[b][2]), fabsf(T4[b][3])), mx);
                    mx = fmaxf(fmaxf(fabsf(T2[b][0]), fabsf(T2[b][1])), mx);
                }
                unsigned mb = __builtin_bit_cast(unsigned, mx);          // non-negative floats order as their bit patterns
                const u32x2 h16 = __builtin_amdgcn_permlane16_swap(mb, mb, false, false);      // {rows 0 0 2 2, rows 1 1 3 3} of mb
                mb = h16[0] > h16[1] ? h16[0] : h16[1];
                const u32x2 h32 = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);      // {halves 0 0, halves 1 1}
                mb = h32[0] > h32[1] ? h32[0] : h32[1];
                unsigned s_bits, inv_bits;
                split2h_scale(mb, SPLIT2H_SAMPLE_TOP, SPLIT2H_SAMPLE_LO, s_bits, inv_bits);
                const float s = __builtin_bit_cast(float, s_bits);
                inv_s[a] = __builtin_bit_cast(float, inv_bits) * inv_t;
#pragma unroll
                for (int b = 0; b < 4; ++b) { T4[b] *= s; T2[b] *= s; }          // exact
            }
            V4[0] = T4[0] - T4[2]; V4[1] = T4[1] + T4[2]; V4[2] = T4[2] - T4[1]; V4[3] = T4[1] - T4[3];
            V2[0] = T2[0] - T2[2]; V2[1] = T2[1] + T2[2]; V2[2] = T2[2] - T2[1]; V2[3] = T2[1] - T2[3];
        };
        // output transform of point (a, b) with accumulators m: along b into Z, at b == 3 along a into Y
        auto consume = [&](int a, int b, const f32x4 (&m)[2]) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                if (b == 0) Z0[nt] = m[nt];
                else if (b == 1) { Z0[nt] += m[nt]; Z1[nt] = m[nt]; }
                else if (b == 2) { Z0[nt] += m[nt]; Z1[nt] -= m[nt]; }
                else if constexpr (F16) {
                    // the row's products carry its scale and the layer's: Z / (s t) is exact, so each sum below rounds once, as the plain sums do
                    Z1[nt] -= m[nt];
                    const float iv = inv_s[a];
                    f32x4 &y00 = Y[0][0][nt], &y01 = Y[0][1][nt], &y10 = Y[1][0][nt], &y11 = Y[1][1][nt];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float z0 = Z0[nt][r], z1 = Z1[nt][r];
                        if (a == 0) { y00[r] = z0 * iv; y01[r] = z1 * iv; }
                        else if (a == 1) { y00[r] = fmaf(z0, iv, y00[r]); y01[r] = fmaf(z1, iv, y01[r]); y10[r] = z0 * iv; y11[r] = z1 * iv; }
                        else if (a == 2) { y00[r] = fmaf(z0, iv, y00[r]); y01[r] = fmaf(z1, iv, y01[r]); y10[r] = fmaf(-z0, iv, y10[r]); y11[r] = fmaf(-z1, iv, y11[r]); }
                        else { y10[r] = fmaf(-z0, iv, y10[r]); y11[r] = fmaf(-z1, iv, y11[r]); }
                    }
                } else {
                    Z1[nt] -= m[nt];
                    if (a == 0) { Y[0][0][nt] = Z0[nt]; Y[0][1][nt] = Z1[nt]; }
                    else if (a == 1) { Y[0][0][nt] += Z0[nt]; Y[0][1][nt] += Z1[nt]; Y[1][0][nt] = Z0[nt]; Y[1][1][nt] = Z1[nt]; }
                    else if (a == 2) { Y[0][0][nt] += Z0[nt]; Y[0][1][nt] += Z1[nt]; Y[1][0][nt] -= Z0[nt]; Y[1][1][nt] -= Z1[nt]; }
                    else { Y[1][0][nt] -= Z0[nt]; Y[1][1][nt] -= Z1[nt]; }
                }
            }
        };
        make_v(0);                                           // sample rows 0 and 2 (requested under the previous group, like row 1)
        // Software pipeline over the 16 points: the MFMA phase of point xi carries, two vector instructions behind each MFMA (the part
        // of an MFMA's 16 cycles in which the vector issue port is free), the truncation residuals of point xi + 1; the tail of the
        // phase requests the weights of xi + 1, packs its three operand quads, and transforms the accumulators of xi.
        if constexpr (F16) {
        // The fp16 form of the same pipeline: per point 4 weight reads, 6 MFMAs (per N tile h2 g1, then h1 g2, then h1 g1: small terms
        // first, the big term rounded once) and, behind the MFMAs, the split of point xi + 1 into its two operand quads
        // (3 v_cvt_pk_f16_f32 + 6 v_cvt_f32_f16 + 6 v_sub_f32 + 3 v_cvt_pk_f16_f32 for six values: 3 per value, and with the scaling of
        // T in make_v 4).  MIX: 3 v_cvt_pk_f16_f32 + 6 v_fma_mix_f32 + 3 v_cvt_pk_f16_f32: 2 per value, 3 with the scaling.
        u32x4 U[2][2];
        u32x4 P1, P2, N1, N2;
        auto split = [&](int b, u32x4 &Q1, u32x4 &Q2) {
            if constexpr (MIX) split2h_6m(V4[b], V2[b], one, Q1, Q2);
            else split2h_6(V4[b], V2[b], Q1, Q2);
        };
        auto load_u = [&](int xi) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) U[nt][pc] = su4[((xi * 2 + nt) * 2 + pc) * 64];
        };
        load_u(0);
        split(0, P1, P2);
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) {
            const int a = xi >> 2, b = xi & 3;
            __builtin_amdgcn_sched_barrier(0);
            f32x4 m[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            m[0] = mfma16h(U[0][0], P2, m[0]); m[1] = mfma16h(U[1][0], P2, m[1]);
            m[0] = mfma16h(U[0][1], P1, m[0]); m[1] = mfma16h(U[1][1], P1, m[1]);
            m[0] = mfma16h(U[0][0], P1, m[0]); m[1] = mfma16h(U[1][0], P1, m[1]);
            // in the MFMAs' shadows: the pieces of the next point of this row (b < 3: V[b + 1] is there; the next row's V does not exist yet)
            if (b < 3) split(b + 1, N1, N2);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, MIX ? W6_MIX_FILL : 3, 0);      // the vector instructions behind it (12 or 18 in all)
            }
            __builtin_amdgcn_sched_barrier(0);
            if (xi == 3 && weights_pending) {                 // first group of the launch: the rest of the weight copy (rounds 2..7)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                 // B
                weights_pending = false;
            }
            if (xi < 15) load_u(xi + 1);
            if (b == 3 && a < 3) {
                make_v(a + 1);
                if (a == 1) load_row(D, A, 3);               // sample row 2 is dead (rows 1 and 3 make row 3)
                if (a == 2) {
                    const int gn = g + stride;               // as in the three-piece form below
                    set_addr(An, gn < g_last ? gn : g_last);
                    load_row(D, An, 0);
                    load_row(D, An, 2);
                }
                split(0, N1, N2);
            }
            if (xi < 15) { P1 = N1; P2 = N2; }
            consume(a, b, m);
            WSTAMP(gcount == 1 && (xi & 3) == 3, 2 + (xi >> 2));
        }
        } else {
        u32x4 U[2][3];
        u32x4 P1, P2, P3;
        f32x4 r4, t4;
        f32x2 r2, t2;
        auto load_u = [&](int xi) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) U[nt][pc] = su4[((xi * 2 + nt) * 3 + pc) * 64];
        };
        load_u(0);
        r4 = resid(V4[0]); t4 = resid(r4); r2 = resid(V2[0]); t2 = resid(r2);
        P1 = pack6(V4[0], V2[0]); P2 = pack6(r4, r2); P3 = pack6(t4, t2);
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) {
            const int a = xi >> 2, b = xi & 3;
            __builtin_amdgcn_sched_barrier(0);
            f32x4 m[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            // smallest terms first: the large one is rounded once
            m[0] = mfma16(U[0][2], P1, m[0]); m[1] = mfma16(U[1][2], P1, m[1]);
            m[0] = mfma16(U[0][0], P3, m[0]); m[1] = mfma16(U[1][0], P3, m[1]);
            m[0] = mfma16(U[0][1], P2, m[0]); m[1] = mfma16(U[1][1], P2, m[1]);
            m[0] = mfma16(U[0][1], P1, m[0]); m[1] = mfma16(U[1][1], P1, m[1]);
            m[0] = mfma16(U[0][0], P2, m[0]); m[1] = mfma16(U[1][0], P2, m[1]);
            m[0] = mfma16(U[0][0], P1, m[0]); m[1] = mfma16(U[1][0], P1, m[1]);
            // in the MFMAs' shadows: residuals of the next point of this row (b < 3: V[b + 1] is there; the next row's V does not exist yet)
            if (b < 3) { r4 = resid(V4[b + 1]); t4 = resid(r4); r2 = resid(V2[b + 1]); t2 = resid(r2); }
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);      // two vector instructions in its shadow
            }
            __builtin_amdgcn_sched_barrier(0);
            // tail: weights of the next point (the MFMAs above have read theirs), its operands, this point's output transform
            if (xi == 3 && weights_pending) {                 // first group of the launch: the rest of the weight copy (rounds 3..11)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                 // B
                weights_pending = false;
            }
            if (xi < 15) load_u(xi + 1);
            if (b == 3 && a < 3) {
                make_v(a + 1);
                if (a == 1) load_row(D, A, 3);               // sample row 2 is dead (rows 1 and 3 make row 3)
                if (a == 2) {
                    // all sample rows are dead: rows 0 and 2 of the next group.  Unconditional (clamped) so that hipcc counts
                    // the outstanding loads exactly.
                    const int gn = g + stride;
                    set_addr(An, gn < g_last ? gn : g_last);
                    load_row(D, An, 0);
                    load_row(D, An, 2);
                }
                r4 = resid(V4[0]); t4 = resid(r4); r2 = resid(V2[0]); t2 = resid(r2);
            }
            if (xi < 15) { const int bn = (b + 1) & 3; P1 = pack6(V4[bn], V2[bn]); P2 = pack6(r4, r2); P3 = pack6(t4, t2); }
            consume(a, b, m);
            WSTAMP(gcount == 1 && (xi & 3) == 3, 2 + (xi >> 2));
        }
        }
        // Row 1 of the NEXT group is requested here, BEFORE this group's stores: the vector-memory counter retires in issue order, so a
        // load issued after the stores is only known to have landed once the stores have been acknowledged -- the wait for row 1 (three
        // points into the next group) then ended with the stores' round trip to L2, ~1 us later than the load itself (the kernel ran
        // in 27.6 us without its stores and 21 us without its loads against 33 us, round 6).  Rows 0 and 2 went out at point 11.
        load_row(D, An, 1);

        // ---- epilogue: lane = (tile i of the group, channel quarter q); registers = 4 consecutive channels.
        // Output (rr, c) is the pixel of sample (row 1 + rr, column 1 + c): its address terms are already there.
        {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    f32x4 v0 = Y[rr][c][0] + bA, v1 = Y[rr][c][1] + bB;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { v0[r] = fmaxf(v0[r], 0.f); v1[r] = fmaxf(v1[r], 0.f); }
                    if constexpr (EPI == 2) {
                        float part = 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) part = fmaf(v0[r], hA[r], part);
#pragma unroll
                        for (int r = 0; r < 4; ++r) part = fmaf(v1[r], hB[r], part);      // hB = 0 for q >= 2
                        part += __shfl_xor(part, 16, 64);                                   // sum over the four channel quarters
                        part += __shfl_xor(part, 32, 64);
                        // logit offset = position * 4: the column term is (oc - 16q) / 24 for lane quarter 0
                        const unsigned lcol = (q == 0 && A.oc[c] != BIG) ? A.oc[c] / (unsigned)UBD_C : BIG;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, part + hbias), yrsrc, (int)(lcol + A.lrow[rr]), 0, 0);
                    } else {
                        const unsigned st1 = (q < 2 && A.oc[c] != BIG) ? A.oc[c] + 64u : BIG;
                        // Stores take the row term in the VECTOR offset: with it in soffset, hipcc's hazard recogniser assumes that a wide
                        // store followed at once by a vector write to its data registers is safe (true of older chips) and inserts no
                        // wait state; on gfx950 ~0.1 % of the pixels of a 32 x 128 x 128 launch then carried a LATER value (an address
                        // integer) in one dword, different ones run to run (tools/wino6_chk_bias.py, round 6).
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v0), yrsrc, (int)(A.oc[c] + A.row[1 + rr]), 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v1), yrsrc, (int)(st1 + A.row[1 + rr]), 0, 0);
                    }
                }
        }
        WSTAMP(gcount == 1, 6);
        WSTAMP(gcount == 0, 1);                              // re-stamped: start of the second group
        ++gcount;
        g += stride;
        if (g >= g_end) break;
        A = An;
    }
    WSTAMP(true, 7);
}

static int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// frag: this layer's slot of packed dwords (UBD_WINO6_SLOT_U32; which form it holds follows h->wino6_split3, as in the pack); epi 0 / 2 as in ubd_launch_dilconv_wino
// lay_in / lay_out: column layout periods of the input and output rows (powers of two, 1: natural; lay_in is 1 or 2 * dilation)
void ubd_launch_dilconv_wino6(const ubd_handle *h, int epi, const unsigned *frag, const float *bias, int dilation,
                              const float *in, float *out, int n, int H4, int W4, hipStream_t st, const float *head,
                              int lay_in, int lay_out)
{
    const int d = dilation;
    const long half_rows = ((H4 + 2 * d - 1) / (2 * d)) * d, half_cols = ((W4 + 2 * d - 1) / (2 * d)) * d;
    // phase grouping: d phases x blocks of 16 of the ceil(W4 / 2d) tiles of a phase
    const long groups_x = lay_in == 1 ? (half_cols + 15) / 16 : (long)d * ((half_cols / d + 15) / 16);
    const long groups = (long)n * half_rows * groups_x;
    w6geom G;
    G.n = n; G.h = H4; G.w = W4; G.d = d; G.log2d = ilog2(d);
    G.phase = lay_in != 1; G.l2po = ilog2(lay_out);
    G.in_bytes = (unsigned)((size_t)n * H4 * W4 * UBD_C * 4);
    G.groups_x = (unsigned)groups_x; G.half_rows = (unsigned)half_rows; G.total = (unsigned)groups;
    // floor(v / D) = (v * m) >> 32 with m = floor((2^32 - 1) / D) + 1, exact while v * D < 2^32: v < groups <= 2^30 / 96 / 4 pixels
    // ... / 16 and D <= 2^12 for every supported shape (tensor bytes <= 2^30); D = 1 needs the identity
    G.magic_gx = groups_x == 1 ? 0u : (unsigned)(0xFFFFFFFFul / (unsigned long)groups_x + 1ul);
    G.magic_hr = half_rows == 1 ? 0u : (unsigned)(0xFFFFFFFFul / (unsigned long)half_rows + 1ul);
    // 64 KiB of LDS (96 KiB for three pieces) and 198-255 registers: one 8-wave block per CU.  A launch with fewer than eight groups per CU (one 512 x 512 image: 256 groups) lets only
    // `wpb` waves of a block take groups, so that the groups spread over all CUs instead of filling 32 of them (batch-1 latency,
    // predict.py:73-78: 10.2 -> 7 us per layer); the other waves still copy their share of the weights and leave.
    int wpb = (int)((groups + h->num_cus - 1) / h->num_cus);
    if (wpb < 1) wpb = 1;
    if (wpb > W6_WAVES) wpb = W6_WAVES;
    G.wpb = wpb;
    int grid = ubd_grid_for(groups, h->num_cus, wpb, 1);
    grid = (grid + 7) / 8 * 8;
    const bool lay = lay_in != 1 || lay_out != 1;
    // three bf16 pieces (UBD_DILCONV=split3) / two fp16 pieces split by conversions (UBD_WINO6_SPLIT=cvt) / by v_fma_mix_f32 (the default)
    auto launch = [&](auto f16_tag, auto mix_tag) {
        constexpr bool F16 = decltype(f16_tag)::value, MIX = decltype(mix_tag)::value;
        if (epi == 2 && lay)
            hipLaunchKernelGGL((dilconv_wino6_kernel<2, true, F16, MIX>), dim3(grid), dim3(64 * W6_WAVES), 0, st, in, out, frag, bias, G, head UBD_STAMP_ARG("wino6"));
        else if (epi == 2)
            hipLaunchKernelGGL((dilconv_wino6_kernel<2, false, F16, MIX>), dim3(grid), dim3(64 * W6_WAVES), 0, st, in, out, frag, bias, G, head UBD_STAMP_ARG("wino6"));
        else if (lay)
            hipLaunchKernelGGL((dilconv_wino6_kernel<0, true, F16, MIX>), dim3(grid), dim3(64 * W6_WAVES), 0, st, in, out, frag, bias, G, nullptr UBD_STAMP_ARG("wino6"));
        else
            hipLaunchKernelGGL((dilconv_wino6_kernel<0, false, F16, MIX>), dim3(grid), dim3(64 * W6_WAVES), 0, st, in, out, frag, bias, G, nullptr UBD_STAMP_ARG("wino6"));
    };
    if (h->wino6_split3) launch(std::false_type{}, std::false_type{});
    else if (h->wino6_cvt_split) launch(std::true_type{}, std::false_type{});
    else launch(std::true_type{}, std::true_type{});
}
