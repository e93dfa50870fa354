// Backward pass of the train step with fp32 gradient tensors between the layers: fp32 and fp16 activations (bwd_pass::backward_f32<TX>).
//
// Notation: layer output Y = relu(Z); G = dL/dZ ("masked" gradient); the kernels pass G tensors from layer to layer:
//   head_dx      G9 = (dlogits . hk^T) * (A9 > 0)
//   dil_wgrad    dW[t][ci][co] = sum_p X[p+off_t][ci] G[p][co], db = sum_p G (MFMA, K-dim = pixels,
//                M = 216 (+1 row of ones for the bias), N = 24)
//   dilconv<1>   G_below = conv(G, flipped/transposed W, same dilation) * (X > 0)   (forward kernel)
//   sep_bwd      separable layer: recomputes the depthwise output, dpw/db (MFMA), dDW = G pw^T (MFMA,
//                lands directly in the depthwise lane layout), ddw (VALU), writes dDW
//   sep_dx       G_below = depthwise-transpose(dDW) * (X > 0)
// The head's weight gradient and the partial sums of every weight gradient: bwd_common.h.
#include "bwd_common.h"

// ------------------------------------------------------------------------------------ backward weight fragments (pack.h)
__global__ void pack_bwd_kernel(const float *__restrict__ params, float *__restrict__ out, pack_bwd_args a)
{
    pack_bwd_body(params, out, a, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}

// ------------------------------------------------------------------------------------ head
template <typename TX>
__global__ __launch_bounds__(256) void head_dx_kernel(const float *__restrict__ dlogits, const void *__restrict__ a9,
                                                      const float *__restrict__ hk, float *__restrict__ g, long npix, int k_out)
{
    __shared__ __attribute__((aligned(16))) float s_kT[(UBD_MAX_CLASSES + 1) * UBD_C];     // head kernel transposed: [k][c]
    for (int t = threadIdx.x; t < UBD_C * k_out; t += blockDim.x) { const int c = t / k_out, k = t - c * k_out; s_kT[k * UBD_C + c] = hk[t]; }
    __syncthreads();
    // one 4-channel chunk per thread: the 16-byte stores (and the activation loads) of a wave are contiguous
    f32x4 *pg = (f32x4 *)g;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < npix * 6; t += (long)gridDim.x * blockDim.x) {
        const long p = t / 6;
        const int c4 = (int)(t - p * 6);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < k_out; ++k) {
            const float dl = dlogits[p * k_out + k];
            const f32x4 wv = *(const f32x4 *)&s_kT[k * UBD_C + c4 * 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(dl, wv[e], acc[e]);
        }
        float av[4];
        if constexpr (sizeof(TX) == 4) {
            const f32x4 a = ((const f32x4 *)a9)[t];
            av[0] = a[0]; av[1] = a[1]; av[2] = a[2]; av[3] = a[3];
        } else {
            const TX *a = (const TX *)a9 + t * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) av[e] = (float)a[e];
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = av[e] > 0.f ? acc[e] : 0.f;
        pg[t] = o;
    }
}

// ------------------------------------------------------------------------------------ dilated wgrad
// dW[t][ci][co] = sum_p X[p + off_t][ci] G[p][co],  db[co] = sum_p G[p][co].
// GEMM view: M = 216 (+ one all-ones row -> bias gradient, padded to 14 tiles of 16), N = 24 (2 tiles), K = pixels.
// A convolution with dilation d is dense on each of the d x d phase sub-grids, so the work is cut into items
// (image, phase (ry, rx), 8 x 16 tile of the sub-grid): the block copies the X tile with a one-sub-pixel halo
// (10 x 18 pixels spaced d in the image) and the G tile into LDS by LDS-DMA (per-lane gather addresses,
// double-buffered against the MFMA phase), and all 9 taps x 24 channels of the A operand are then read from LDS
// (ds_read_b32) instead of 14 global gathers per k-step.  Each wave owns every 4th k-step (4 consecutive
// sub-pixels), accumulates the whole 224 x 32 result in 112 VGPRs across all its items, and the block reduces
// through LDS to one fp32 atomic per output at the very end.
#define WG_TH 8
#define WG_TW 16
#define WG_XW (WG_TW + 2)
#define WG_XPIX ((WG_TH + 2) * WG_XW)          // 180
#define WG_GPIX (WG_TH * WG_TW)                // 128
#define WG_ROUNDS 8                            // (180 * 6 + 128 * 6 + 255) / 256 with fp32 activations (7 with 16-bit)
#define WG_BUF_FLOATS (WG_ROUNDS * 256 * 4)    // 8192 floats = 32 KiB

// MS = 2 (round 5, fp32 activations): the block has EIGHT waves -- wave (ks = wid & 3, mh = wid >> 2) takes the k-steps ks, ks + 4, ... like
// before but only the seven M tiles 7 mh .. 7 mh + 6 of them (56 accumulator registers instead of 112, < 128 in all): two blocks per CU are
// then four waves per SIMD, where the fp32 MFMA issues every ~20 cycles per SIMD instead of every ~25-32 at two (tools/ubench/mfma_fill.hip).
// The sums are the same numbers added in the same order (k-step classes 0..3 per accumulator tile): bit-identical to MS = 1.
template <typename TX, int MS = 1>
__global__ __launch_bounds__(256 * MS, 2 * MS) void dil_wgrad_kernel(const void *__restrict__ x, const float *__restrict__ gz,
                                                           float *__restrict__ partials, int n, int h,
                                                           int w, int d)
{
    constexpr int NTH = 256 * MS, MT = 14 / MS;                    // threads per block, M tiles per wave
    __shared__ __attribute__((aligned(16))) float smem[2 * WG_BUF_FLOATS];     // 64 KiB: two tile buffers / final reduction
    __shared__ TX s_one[4];                                                     // 1.0: the A value of the ones row (bias gradient)
    if (threadIdx.x < 4) s_one[threadIdx.x] = (TX)1.f;                          // visible after the first item's barrier
    const int lane = threadIdx.x & 63, m = lane & 15, k = lane >> 4;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ks = wid & 3, mh = wid >> 2;                         // k-step class, M half (MS = 1: mh = 0)
    constexpr int XCH = (int)sizeof(TX) * UBD_C / 16;              // 16-byte chunks per X pixel: 6 (fp32) or 3 (16-bit)
    constexpr int WG_CHUNKS = WG_XPIX * XCH + WG_GPIX * 6;
    constexpr int XBYTES = WG_XPIX * UBD_C * (int)sizeof(TX);      // G tile starts here (multiple of 16)

    // A-operand rows of the 14 M-tiles: dword offset of (tap, ci) relative to the X-tile pixel of the output position
    int aoff[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int rho = 16 * (mt + mh * MT) + m;
        const int t = rho / UBD_C, ci = rho % UBD_C;
        aoff[mt] = ((t / 3) * WG_XW + (t % 3)) * UBD_C + ci;          // rows >= 216 are never read (see below)
    }
    // the last M tile (rows 208..223) holds 8 real rows, the ones row (bias gradient) and zeros: only the wave that owns it treats it specially
    const bool last_tile = mh == MS - 1;                                        // wave-uniform
    const bool row13_real = !last_tile || m < 8, row13_ones = last_tile && m == 8;
    const int aoff13c = row13_real ? aoff[MT - 1] : aoff[MT - 2];               // a valid offset for every lane (rows >= 216 read a neighbour's, unused)

    // work items
    const int sh = (h + d - 1) / d, sw = (w + d - 1) / d;              // largest sub-grid
    const int tiles_y = (sh + WG_TH - 1) / WG_TH, tiles_x = (sw + WG_TW - 1) / WG_TW;
    const int items = n * d * d * tiles_y * tiles_x;

    struct item_t { int img, ry, rx, sy0, sx0; };
    auto decode = [&](int it) {
        item_t r;
        const int tx = (int)((unsigned)it % (unsigned)tiles_x); it = (int)((unsigned)it / (unsigned)tiles_x);
        const int ty = (int)((unsigned)it % (unsigned)tiles_y); it = (int)((unsigned)it / (unsigned)tiles_y);
        r.rx = (int)((unsigned)it % (unsigned)d); it = (int)((unsigned)it / (unsigned)d);
        r.ry = (int)((unsigned)it % (unsigned)d);
        r.img = (int)((unsigned)it / (unsigned)d);
        r.sy0 = ty * WG_TH; r.sx0 = tx * WG_TW;
        return r;
    };
    // chunk c of the combined tile: c < XPIX*6 -> X pixel (with halo), else G pixel; returns image coords
    // chunk c of the combined tile: X pixels (with halo, XCH chunks each) first, then G pixels (6 chunks each)
    auto chunk_src = [&](const item_t &I, int c, bool &is_x, int &gy, int &gx, int &part) {
        c = c < WG_CHUNKS ? c : WG_CHUNKS - 1;
        is_x = c < WG_XPIX * XCH;
        int sy, sx;
        if (is_x) { const int pix = c / XCH; part = c - pix * XCH; sy = pix / WG_XW - 1; sx = pix % WG_XW - 1; }
        else { const int cg = c - WG_XPIX * XCH; const int gp = cg / 6; part = cg - gp * 6; sy = gp / WG_TW; sx = gp % WG_TW; }
        gy = I.ry + (I.sy0 + sy) * d;
        gx = I.rx + (I.sx0 + sx) * d;
    };
    // which pixel / 16-byte part a thread moves in round rd does not depend on the item: decoded ONCE (the divisions by 6, 18, 16 per round
    // and item were ~100 of the ~500 non-MFMA instructions a wave spends per item; round 5)
    constexpr int ROUNDS = (WG_CHUNKS + NTH - 1) / NTH;
    int cpk[ROUNDS];                                                   // (sy + 1) | (sx + 1) << 8 | part << 16 | is_x << 24
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        int c = rd * NTH + (int)threadIdx.x;
        c = c < WG_CHUNKS ? c : WG_CHUNKS - 1;
        const bool is_x = c < WG_XPIX * XCH;
        int sy, sx, part;
        if (is_x) { const int pix = c / XCH; part = c - pix * XCH; sy = pix / WG_XW - 1; sx = pix % WG_XW - 1; }
        else { const int cg = c - WG_XPIX * XCH; const int gp = cg / 6; part = cg - gp * 6; sy = gp / WG_TW; sx = gp % WG_TW; }
        cpk[rd] = (sy + 1) | ((sx + 1) << 8) | (part << 16) | ((is_x ? 1 : 0) << 24);
    }
    const unsigned lds_smem = ubd_lds_addr(smem);
    auto dma_item = [&](int it, int buf_floats) {
        const item_t I = decode(it);
        const char *xim = (const char *)x + (size_t)I.img * h * w * (UBD_C * sizeof(TX));
        const char *gim = (const char *)gz + (size_t)I.img * h * w * (UBD_C * sizeof(float));
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            const int cbase = rd * NTH + wid * 64;
            const int pk = cpk[rd];
            const int sy = (pk & 255) - 1, sx = ((pk >> 8) & 255) - 1, part = (pk >> 16) & 255;
            const bool is_x = (pk >> 24) != 0;
            int gy = I.ry + (I.sy0 + sy) * d, gx = I.rx + (I.sx0 + sx) * d;
            gy = gy < 0 ? 0 : (gy >= h ? h - 1 : gy);                 // clamped; out-of-image pixels are zeroed later
            gx = gx < 0 ? 0 : (gx >= w ? w - 1 : gx);
            const unsigned pixel = (unsigned)(gy * w + gx);
            const char *src = is_x ? xim + (size_t)pixel * (UBD_C * sizeof(TX)) + part * 16
                                   : gim + (size_t)pixel * (UBD_C * sizeof(float)) + part * 16;
            // the asm form (common.h): hipcc orders every LDS read behind a builtin LDS-DMA in flight (s_waitcnt vmcnt(0) in front of the
            // first operand load), which put the next item's whole fetch in front of this item's MFMAs (round 5: 161 -> see DESIGN 5.4)
            ubd_glds16_at(src, lds_smem + (unsigned)(buf_floats + cbase * 4) * 4u);
        }
    };

    // XCD-aware item ranges (see dil_wgrad16_kernel): the phases of one image go through ONE L2
    const int xcd = blockIdx.x & 7;
    const int nblk_x = ((int)gridDim.x + 7 - xcd) >> 3;
    const int chunk = (items + 7) >> 3;
    const int it_begin = xcd * chunk;
    const int it_end = it_begin + chunk < items ? it_begin + chunk : items;
    f32x4 acc[MT][2] = {};
    int it = it_begin + (int)(blockIdx.x >> 3);
    if (it < it_end) dma_item(it, 0);
    for (int iter = 0; it < it_end; ++iter, it += nblk_x) {
        float *buf = smem + (iter & 1) * WG_BUF_FLOATS;
        const item_t I = decode(it);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this item's DMA (issued one item ago, as asm) has landed
        __syncthreads();                              // ... for every wave; everyone left the other buffer
        if (it + nblk_x < it_end) dma_item(it + nblk_x, ((iter + 1) & 1) * WG_BUF_FLOATS);
        // zero the pixels that lie outside the image (halo / ragged sub-grid edge)
        const bool ragged = (I.ry + (I.sy0 - 1) * d < 0) || (I.rx + (I.sx0 - 1) * d < 0) ||
                            (I.ry + (I.sy0 + WG_TH) * d >= h) || (I.rx + (I.sx0 + WG_TW) * d >= w);   // block-uniform
        if (ragged) {
            for (int pix = threadIdx.x; pix < WG_XPIX + WG_GPIX; pix += NTH) {
                bool is_x; int gy, gx, part;
                const bool xp_ = pix < WG_XPIX;
                chunk_src(I, xp_ ? pix * XCH : WG_XPIX * XCH + (pix - WG_XPIX) * 6, is_x, gy, gx, part);
                if (gy < 0 || gy >= h || gx < 0 || gx >= w) {
                    f32x4 *z = (f32x4 *)((char *)buf + (xp_ ? pix * UBD_C * (int)sizeof(TX) : XBYTES + (pix - WG_XPIX) * UBD_C * 4));
                    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                    const int nq = xp_ ? XCH : 6;
                    for (int q6 = 0; q6 < nq; ++q6) z[q6] = zero;
                }
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_s_barrier();             // raw barrier: the next item's DMA stays in flight
        }
        // k-steps: (row py, group of 4 consecutive sub-pixels); this wave takes every 4th
        const int rows_eff = min(WG_TH, sh - I.sy0), grp_eff = (min(WG_TW, sw - I.sx0) + 3) >> 2;
        const int nsteps = rows_eff * grp_eff;
        const TX *xt = (const TX *)buf;
        const float *gt = (const float *)((const char *)buf + XBYTES);
        // operands of k-step s (14 A values: (tap, ci) rows of the lane's sub-pixel; 2 B values: its gradient channels); the loads of
        // step s + 4 are issued in front of the 28 MFMAs of step s (round 5: the wave used to wait for every step's LDS round trip)
        auto ld_step = [&](int s, float (&a)[MT], float &b0, float &b1) {
            const int py = (int)((unsigned)s / (unsigned)grp_eff), pg = s - py * grp_eff;
            const int px = pg * 4 + k;                                 // this lane's sub-pixel column
            const TX *xp = xt + (py * WG_XW + px) * UBD_C;             // X-tile pixel of tap (0,0)
            const float *gp = gt + (py * WG_TW + px) * UBD_C;
            // every load unconditional and NO select after a load: an exec-masked load or a v_cndmask on a loaded value sits in the block
            // of the loads, and hipcc then waits for all of them (lgkmcnt(0)) before the MFMAs of the step in front -- the prefetch
            // would be gone.  Lanes without a value read a finite neighbour's: columns >= 8 of the second N tile and rows >= 217 are never
            // stored (wgrad_block_reduce), and the ones row (bias gradient) reads a 1.0 kept in LDS (the select is on the ADDRESS).
            b0 = gp[m];
            b1 = gp[16 + (m & 7)];
#pragma unroll
            for (int mt = 0; mt < MT - 1; ++mt) a[mt] = (float)xp[aoff[mt]];
            const TX *p13 = row13_ones ? (const TX *)s_one : xp + aoff13c;
            a[MT - 1] = (float)*p13;
        };
        float a0[MT], a1[MT], b00 = 0.f, b01 = 0.f, b10 = 0.f, b11 = 0.f;
        int s = ks;
        if (s < nsteps) ld_step(s, a0, b00, b01);
        for (; s < nsteps; s += 8) {
            if (s + 4 < nsteps) ld_step(s + 4, a1, b10, b11);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[mt], b00, acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[mt], b01, acc[mt][1], 0, 0, 0);
            }
            if (s + 4 >= nsteps) break;
            if (s + 8 < nsteps) ld_step(s + 8, a0, b00, b01);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[mt], b10, acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[mt], b11, acc[mt][1], 0, 0, 0);
            }
        }
    }
    wgrad_block_reduce<MT>(acc, smem, partials + (size_t)blockIdx.x * (217 * UBD_C), lane, ks, mh * MT);
}

// ------------------------------------------------------------------------------------ separable backward
// Persistent blocks over output tiles of 16 columns x TH rows (as the forward sepconv_kernel): the input
// patch and the G tile are staged in LDS (24 channels: LDS-DMA, clamped + zero-fixed at the image border;
// 1/3 channels: converted on the way through registers), every tap and both G layouts are then read from LDS.
template <int CIN, int STRIDE, int XB, int UPS = 0> struct sepb_cfg {          // XB = bytes per element of a 24-channel input
    // 1/3-channel layer with the in-block G tile (fp32 gradient path): 8-row tiles, 40 KB of LDS -- FOUR blocks per CU instead of two (the
    // kernel waited for memory two thirds of its time, PMC round 5)
    static constexpr int TH = ((CIN == UBD_C && STRIDE == 2) || (CIN != UBD_C && UPS > 0)) ? 8 : 16;
    static constexpr int PH = (TH - 1) * STRIDE + 3;
    static constexpr int PW = 15 * STRIDE + 3;
    static constexpr int XPIX = PH * PW;
    static constexpr int GPIX = TH * 16;
    static constexpr int XCH = XB * UBD_C / 16;                                        // DMA chunks per X pixel
    // LDS layout of the fp32 tiles (round 5).  A lane (pixel i, channel group q) reads 8-byte pairs at pixel_position + 6 q: at 24 dwords
    // per pixel, pixels i and i + 8 (stride 1) or i and i + 4, 8, 12 (stride 2) start in the same bank, every read took 2 (4) passes and
    // the LDS pipe was busy 54 % of the 24-channel kernel's time, 59 % of that in bank conflicts (profiles/r05_pmc_sep_bwd32.txt).
    // The LDS-DMA lands 16-byte chunks at consecutive slots, WHICH chunk a slot fetches is free -- so a pad chunk is left out:
    //   G tile, X patch of a stride-1 layer: 7 slots (28 dwords) per pixel; X patch of a stride-2 layer: 13 slots per PAIR of pixels.
    // Then the 32 lanes of a half-wave read 64 different banks (tools/lds_bank_model.py).
    static constexpr bool XSW = (CIN == UBD_C) && XB == 4;
    static constexpr int XROW_CH = !XSW ? PW * XCH : (STRIDE == 1 ? PW * 7 : (PW / 2) * 13 + (PW % 2) * 6);   // slots per X patch row
    static constexpr int XROW_DW = XROW_CH * 4;
    __host__ __device__ static constexpr int xpos_dw(int pc)                           // dword offset of pixel column pc in its row
    {
        return !XSW ? pc * (UBD_C * XB / 4) : (STRIDE == 1 ? pc * 28 : pc * 24 + (pc >> 1) * 4);
    }
    static constexpr int GPIX_DW = 28;                                                 // G tile: dwords per pixel
    // 1/3-channel patch: rows of XROW_E floats = whole 16-byte chunks with room for the skew between a chunk boundary and the patch's first float
    static constexpr int XROWC = (PW * CIN + 3 + 3) / 4, XROW_E = XROWC * 4;
    static constexpr int XFLOATS = (CIN == UBD_C) ? PH * XROW_DW : PH * XROW_E;
    static constexpr int XCHUNKS = (CIN == UBD_C) ? PH * XROW_CH : 0;
    static constexpr int GCHUNKS = GPIX * 7;                                           // a multiple of 64: every wave's 64 slots lie in ONE region
    static constexpr int CHUNKS = GCHUNKS + XCHUNKS;                                   // DMA slots: the G tile, then (24 channels) the X patch
    static constexpr int ROUNDS = (CHUNKS + 255) / 256;
    static constexpr int GOFF = (CIN == UBD_C) ? 0 : XFLOATS;                          // float offset of the DMA region
    static constexpr int LDS_FLOATS = GOFF + CHUNKS * 4;                               // exact: slots past CHUNKS are not fetched
};

// TX: element type of a 24-channel input patch; TR: activation type of the model (16-bit: kernels and the depthwise
// output are used rounded to TR, as in the forward pass)
// UPS > 0 (round 5, fp32 gradient path): the G tile is COMPUTED in the block instead of being read -- `G` then points at this layer's own
// output activation (the ReLU mask source, same shape as G), `up_ddw` at the dDW tensor of the layer above (stride UPS, top/left padding
// up_pad, map up_oh x up_ow) and `up_dw` at that layer's depthwise kernel [9][24]:
//     G[p][c] = (A[p][c] > 0) * sum_t dDW_up[(p + up_pad - t) / UPS][c] * dw_up[t][c]        (taps in sep_dx_kernel's order: the same bits)
// i.e. sep_dx_kernel's arithmetic on the tile, so that kernel's launch -- 403 MB read + 403 MB mask + 403 MB written per separable
// layer at 64 images -- and the G tensor itself disappear.
// diagnostic build only (stamps.h): the phase boundaries, every wave, first 8 tiles of the block, 12 slots per tile (tools/stamps_sepb32.py)
#define SB32STAMP(k) UBD_STAMP(stamp_it < 8, (((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + stamp_it) * 12 + (k))
template <int CIN, int STRIDE, int IN_U8, typename TX, typename TR, int UPS = 0>
__global__ __launch_bounds__(256, (CIN != UBD_C && UPS > 0) ? 4 : 2) void sep_bwd_kernel(const void *__restrict__ xin, const float *__restrict__ G,
                                                      float *__restrict__ dDW, const float *__restrict__ fwdfrag,
                                                      const float *__restrict__ bwdfrag, float *__restrict__ partials, int n, int H, int W,
                                                      int OH, int OW, int pad_lo, float pre_sub, float pre_div,
                                                      const float *__restrict__ up_ddw = nullptr, const float *__restrict__ up_dw = nullptr,
                                                      int up_oh = 0, int up_ow = 0, int up_pad = 0 UBD_STAMP_PARAM)
{
    using C = sepb_cfg<CIN, STRIDE, (int)sizeof(TX), UPS>;
    static_assert(UPS == 0 || sizeof(TX) == 4 || CIN != UBD_C, "the in-block G tile needs an fp32 mask tile of G's size");
    constexpr int UPH = UPS == 1 ? C::TH + 2 : C::TH / 2 + 2, UPW = UPS == 1 ? 18 : 10;      // patch of the upper layer's dDW
    __shared__ __attribute__((aligned(16))) float s_up[UPS > 0 ? UPH * UPW * UBD_C + 9 * UBD_C : 4];
    constexpr int CPL = (CIN == UBD_C) ? 6 : 1;
    constexpr int NT_A = (CIN == UBD_C) ? 2 : 1;           // tiles of the dDW product
    constexpr int MT_PW = (CIN == UBD_C) ? 2 : 1;          // M tiles of the dpw product (CIN rows + ones row)
    __shared__ __attribute__((aligned(16))) float lds[C::LDS_FLOATS];
    __shared__ float s_dw[4][16][CIN == UBD_C ? UBD_C : 4];           // depthwise output of a row, transposed for the dpw product (columns = channels)
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = lane & 15, q = lane >> 4;
    const float *dwlane = fwdfrag + UBD_SEP_FRAG_FLOATS;
    float *gtile = lds + C::GOFF;                                       // DMA region: G tile, then the 24-channel X patch
    float *xpatch = (CIN == UBD_C) ? gtile + C::GCHUNKS * 4 : lds;
    const unsigned lds_dma = ubd_lds_addr(lds) + C::GOFF * 4u;             // LDS byte address of DMA slot 0

    float dwk[9][CPL];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s = 0; s < CPL; ++s) dwk[t][s] = rnd_act<TR>(dwlane[(t * 6 + s) * 64 + lane]);
    float apw[6][NT_A];
#pragma unroll
    for (int s = 0; s < 6; ++s)
#pragma unroll
        for (int tl = 0; tl < NT_A; ++tl) apw[s][tl] = rnd_act<TR>(bwdfrag[(s * 2 + tl) * 64 + lane]);
    const bool ch_ok = (CIN == UBD_C) || (q < CIN);
    const int cb = (CIN == UBD_C) ? 6 * q : (q < CIN ? q : 0);

    float ddw[9][CPL];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s = 0; s < CPL; ++s) ddw[t][s] = 0.f;
    f32x4 accpw[MT_PW][2] = {};

    const int tiles_x = (OW + 15) >> 4, tiles_y = (OH + C::TH - 1) / C::TH;
    const int total = n * tiles_y * tiles_x;
    ubd_tile_decoder tdec;
    tdec.init(tiles_x, tiles_y, total);
    [[maybe_unused]] int stamp_it = -1;
    const unsigned lds_up = ubd_lds_addr(s_up);
    if constexpr (UPS > 0) {
        if (threadIdx.x < 9 * UBD_C) s_up[UPH * UPW * UBD_C + threadIdx.x] = rnd_act<TR>(up_dw[threadIdx.x]);     // the upper layer's depthwise kernel: visible after the first tile's barrier
    }
    // 1/3-channel fp32 input whose rows are whole 16-byte chunks: fetched 16 bytes per lane (see the staging); xsk = floats between a chunk
    // boundary and the patch's first float
    const bool xwide = (CIN != UBD_C) && !IN_U8 && ((W * CIN) & 3) == 0 && ((uintptr_t)xin & 15) == 0 && (unsigned long long)H * W * CIN * 4 < (1ull << 31);   // 16-byte loads: aligned base, rows of whole chunks
    const int xsk = xwide ? ((-(CIN * pad_lo)) & 3) : 0;
    for (int ltile = blockIdx.x; ltile < total; ltile += gridDim.x) {
        int tx, ty, img;
        tdec.decode(ltile, tx, ty, img);                                   // neighbouring tiles on one XCD (shared halo lines)
        const int oy0 = ty * C::TH, ox0 = tx * 16;
        const int ix0 = ox0 * STRIDE - pad_lo, iy0 = oy0 * STRIDE - pad_lo;
        ++stamp_it;
        SB32STAMP(0);
        __syncthreads();                                               // previous tile fully consumed
        SB32STAMP(1);
        // the staging below decodes slot / element numbers that depend on the thread only: opaque per tile, or hipcc computes the decode of every
        // round once, in front of the tile loop, and parks it in scratch (27 spilled registers at the 128 of the four-blocks-per-CU variants)
        int lane_o = lane, tid_o = (int)threadIdx.x;
        asm volatile("" : "+v"(lane_o), "+v"(tid_o));
        // ---- stage X patch (24 ch) and G tile by LDS-DMA; clamped addresses, zero-fix below
        // Every wave-round fetches 64 consecutive slots of ONE region; (row, slot in the row) of its first slot are scalar arithmetic, a lane adds
        // its number and wraps into the next row at most once (rows are >= 64 slots), small divisions are one multiply, the address is a scalar
        // image base + a 32-bit lane offset (the launcher checks that an image fits).  Round 5: with one flat slot number per lane decoded by
        // 32-bit divisions and a 64-bit address per lane a round cost ~500 cycles of (mostly quarter-rate) VALU -- 7500 of the 24-channel
        // tile's 40000 (profiles/r05_stamps_sepb32.txt).
        static_assert(C::GCHUNKS % 64 == 0 && 16 * 7 >= 64 && (CIN != UBD_C || C::XROW_CH >= 64 || !C::XSW), "one region, one wrap per wave-round");
        const char *xim = (const char *)xin + (size_t)img * H * W * (UBD_C * sizeof(TX));     // wave-uniform bases
        const char *gim = (const char *)G + (size_t)img * OH * OW * (UBD_C * sizeof(float));
#pragma unroll 2
        for (int rd = 0; rd < C::ROUNDS; ++rd) {
            const int cbase = rd * 256 + wid * 64;
            if (cbase >= C::CHUNKS) break;                             // wave-uniform
            const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_dma + (unsigned)cbase * 16u));
            if (cbase < C::GCHUNKS) {
                const int row0 = cbase / 112;                          // scalar
                int rc = cbase - row0 * 112 + lane_o;
                const int wrap = rc >= 112 ? 1 : 0;
                rc -= wrap * 112;
                const int px = (rc * 147) >> 10, part = rc - px * 7;   // rc / 7 for rc < 209
                int gy = oy0 + row0 + wrap, gx = ox0 + px;
                gy = gy >= OH ? OH - 1 : gy;
                gx = gx >= OW ? OW - 1 : gx;
                const unsigned off = (unsigned)(gy * OW + gx) * (unsigned)(UBD_C * 4) + (unsigned)(part * 16);
                if (part < 6) ubd_glds16_sbase(gim, off, dst);
            } else if constexpr (CIN == UBD_C) {
                const int cx = cbase - C::GCHUNKS;
                int pr, pc, part;
                bool fetch;
                if constexpr (C::XSW) {
                    const int row0 = cx / C::XROW_CH;                  // scalar
                    int rc = cx - row0 * C::XROW_CH + lane_o;
                    const int wrap = rc >= C::XROW_CH ? 1 : 0;
                    rc -= wrap * C::XROW_CH;
                    pr = row0 + wrap;
                    if constexpr (STRIDE == 1) { pc = (rc * 147) >> 10; part = rc - pc * 7; fetch = part < 6; }
                    else {
                        const int pp = (rc * 79) >> 10, r13 = rc - pp * 13;      // rc / 13 for rc < 350: pair of pixels, slot inside (12: the pad)
                        const int hi = r13 >= 6 ? 1 : 0;
                        pc = 2 * pp + hi; part = r13 - 6 * hi; fetch = r13 < 12;
                    }
                } else {
                    const int c = cx + lane_o;
                    pr = c / C::XROW_CH;
                    const int rc = c - pr * C::XROW_CH;
                    pc = rc / C::XCH; part = rc - pc * C::XCH; fetch = true;
                }
                fetch = fetch && pr < C::PH;
                int gy = iy0 + pr, gx = ix0 + pc;
                gy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy);
                gx = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
                const unsigned off = (unsigned)(gy * W + gx) * (unsigned)(UBD_C * sizeof(TX)) + (unsigned)(part * 16);
                if (fetch) ubd_glds16_sbase(xim, off, dst);
            }
        }
        if constexpr (UPS > 0) {
            // ---- the dDW patch of the layer above, by LDS-DMA too (clamped addresses: the G tile below reads a patch pixel only where it lies
            //      inside the upper map).  Round 5: first loaded behind the DMA's barrier (a second memory round trip per tile), then through
            //      registers in flight with the DMA -- 20 registers the four-blocks-per-CU variants do not have.
            const int uy0 = UPS == 1 ? oy0 + up_pad - 2 : ((oy0 + up_pad - 2) >> 1), ux0 = UPS == 1 ? ox0 + up_pad - 2 : ((ox0 + up_pad - 2) >> 1);
            const char *uim = (const char *)up_ddw + (size_t)img * up_oh * up_ow * (UBD_C * 4);
            constexpr int UCH = UPH * UPW * 6;
#pragma unroll
            for (int rd = 0; rd < (UCH + 255) / 256; ++rd) {
                const int cbase = rd * 256 + wid * 64;
                if (cbase >= UCH) break;                               // wave-uniform
                const unsigned c = (unsigned)(cbase + lane_o);
                const unsigned cc = c < (unsigned)UCH ? c : (unsigned)(UCH - 1);
                const unsigned pix = cc / 6u, part = cc - pix * 6u;
                const unsigned pr = pix / (unsigned)UPW, pc = pix - pr * UPW;
                int gy = uy0 + (int)pr, gx = ux0 + (int)pc;
                gy = gy < 0 ? 0 : (gy >= up_oh ? up_oh - 1 : gy);
                gx = gx < 0 ? 0 : (gx >= up_ow ? up_ow - 1 : gx);
                const unsigned off = (unsigned)(gy * up_ow + gx) * (unsigned)(UBD_C * 4) + part * 16u;
                if (c < (unsigned)UCH) ubd_glds16_sbase(uim, off, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_up + (unsigned)cbase * 16u)));
            }
        }
        // small-channel input: through registers (converted on the way).  All of a thread's loads first (unconditional), the LDS stores behind
        // the upper patch's below: as a load -> store loop of seven trips this was 7 memory round trips per tile.  fp32 rows that are a whole
        // number of 16-byte chunks (`xwide`): 16 bytes per lane -- chunks left / right of the row or above / below the image are outside as a
        // whole and become zeros -- 7 wave-loads per tile instead of 27 (the vector memory pipe takes
        // ~170-200 cycles per wave-load whatever its width, tools/ubench/dma_issue.hip); patch rows then start `xsk` floats into their LDS row.
        constexpr int NXR = (CIN != UBD_C) ? (C::XPIX * CIN + 255) / 256 : 1;
        constexpr int NXW = (CIN != UBD_C) ? (C::PH * C::XROWC + 255) / 256 : 1;
        [[maybe_unused]] float xv[IN_U8 ? NXR : 1];
        [[maybe_unused]] f32x4 xw[IN_U8 ? 1 : NXW];
        if constexpr (CIN != UBD_C) {
            if (xwide) {
                // loaded, converted and stored in one piece below
            } else if constexpr (IN_U8) {
                constexpr unsigned ROWE = C::PW * CIN;                 // a patch row is ROWE consecutive elements of the image row
                const size_t ibase = (size_t)img * H * W * CIN;
#pragma unroll
                for (int k = 0; k < NXR; ++k) {
                    const unsigned e = (unsigned)(k * 256 + tid_o);
                    const unsigned ec = e < (unsigned)(C::XPIX * CIN) ? e : (unsigned)(C::XPIX * CIN - 1);
                    const unsigned pr = ec / ROWE, col = ec - pr * ROWE;
                    const unsigned pc = col / (unsigned)CIN, ch = col - pc * CIN;
                    const int gy = iy0 + (int)pr, gx = ix0 + (int)pc;
                    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    const int gyc = gy < 0 ? 0 : (gy >= H ? H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
                    const float raw = (float)((const unsigned char *)xin)[ibase + ((size_t)gyc * W + gxc) * CIN + ch];
                    xv[k] = in ? (raw - pre_sub) / pre_div : 0.f;
                }
            } else {
                // fp32 rows that are no whole number of chunks (W * CIN % 4 != 0): element by element, stored at once (the slow path)
                for (int e = tid_o; e < C::XPIX * CIN; e += 256) {
                    const int pr = e / (C::PW * CIN), col = e - pr * (C::PW * CIN);
                    const int pc = col / CIN, ch = col - pc * CIN;
                    const int gy = iy0 + pr, gx = ix0 + pc;
                    float v = 0.f;
                    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = (((const float *)xin)[(((size_t)img * H + gy) * W + gx) * CIN + ch] - pre_sub) / pre_div;
                    xpatch[pr * C::XROW_E + col] = v;
                }
            }
        }
        if constexpr (CIN != UBD_C) {
            if (xwide) {
                const int a0f = ix0 * CIN - xsk, WC = W * CIN;                 // a0f: a multiple of 4 (tile origins are multiples of 32 pixels)
                const float *xim = (const float *)xin + (size_t)img * H * WC;
                bool okk[NXW];
#pragma unroll
                for (int k = 0; k < NXW; ++k) {
                    const unsigned c = (unsigned)(k * 256 + tid_o);
                    const unsigned pr = c / (unsigned)C::XROWC, pc = c - pr * C::XROWC;
                    const int gy = iy0 + (int)pr, f0 = a0f + 4 * (int)pc;
                    // a chunk is inside the image row or outside as a whole (rows are whole chunks): outside -> any valid address, zeroed below
                    okk[k] = c < (unsigned)(C::PH * C::XROWC) && (unsigned)gy < (unsigned)H && (unsigned)f0 < (unsigned)WC;
                    xw[k] = *(const f32x4 *)(xim + (okk[k] ? gy * WC + f0 : 0));
                }
#pragma unroll
                for (int k = 0; k < NXW; ++k) {
                    const unsigned c = (unsigned)(k * 256 + tid_o);
                    const bool ok = okk[k];                            // else: padding, exactly 0 after the preprocessing too
                    f32x4 v;
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) v[e4] = ok ? (xw[k][e4] - pre_sub) / pre_div : 0.f;
                    if (c < (unsigned)(C::PH * C::XROWC)) *(f32x4 *)(xpatch + c * 4) = v;
                }
            } else if constexpr (IN_U8) {
#pragma unroll
                for (int k = 0; k < NXR; ++k) {
                    const unsigned e = (unsigned)(k * 256 + tid_o);
                    const unsigned pr = e / (unsigned)(C::PW * CIN);
                    if (e < (unsigned)(C::XPIX * CIN)) xpatch[e + pr * (unsigned)(C::XROW_E - C::PW * CIN)] = xv[k];     // rows of XROW_E floats
                }
            }
        }
        SB32STAMP(2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's LDS-DMA has landed (asm form: hipcc keeps no count of it)
        __syncthreads();                                               // ... every wave's; LDS writes visible
        SB32STAMP(3);
        {
            const bool xborder = (CIN == UBD_C) && ((iy0 < 0) || (ix0 < 0) || (iy0 + C::PH > H) || (ix0 + C::PW > W));
            const bool gborder = (oy0 + C::TH > OH) || (ox0 + 16 > OW);
            if (xborder || gborder) {                                  // block-uniform
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                if (xborder)
                    for (int pix = threadIdx.x; pix < C::XPIX; pix += 256) {
                        const int pr = pix / C::PW, pc = pix - pr * C::PW;
                        const int gy = iy0 + pr, gx = ix0 + pc;
                        if (gy < 0 || gy >= H || gx < 0 || gx >= W) {
                            f32x4 *z = (f32x4 *)(xpatch + pr * C::XROW_DW + C::xpos_dw(pc));
#pragma unroll
                            for (int k6 = 0; k6 < C::XCH; ++k6) z[k6] = zero;
                        }
                    }
                if (gborder)
                    for (int pix = threadIdx.x; pix < C::GPIX; pix += 256)
                        if (oy0 + (pix >> 4) >= OH || ox0 + (pix & 15) >= OW) {
                            f32x4 *z = (f32x4 *)(gtile + pix * C::GPIX_DW);
#pragma unroll
                            for (int k6 = 0; k6 < 6; ++k6) z[k6] = zero;
                        }
                __syncthreads();
            }
        }

        SB32STAMP(4);
        if constexpr (UPS > 0) {
            // ---- the G tile from the layer above: its dDW patch (zeros outside its map) and its depthwise kernel into LDS, then every
            //      thread turns six 4-channel chunks of the mask tile into G in place
            float *upk = s_up + UPH * UPW * UBD_C;
            const int uy0 = UPS == 1 ? oy0 + up_pad - 2 : ((oy0 + up_pad - 2) >> 1), ux0 = UPS == 1 ? ox0 + up_pad - 2 : ((ox0 + up_pad - 2) >> 1);
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            // Tiles all of whose taps lie inside the upper map (all but the map's border tiles; block-uniform): no bounds, no clamps -- a chunk's
            // patch and weight addresses are ONE base each plus compile-time offsets (stride 2: the parity of the pixel is in the bases, a tap with
            // ky or kx = 3 is switched off by a select).  Same taps, same order, same sums as the general loop below.
            const bool interior = oy0 + up_pad - 2 >= 0 && ox0 + up_pad - 2 >= 0 && (oy0 + up_pad + C::TH - 1) / UPS < up_oh && (ox0 + up_pad + 15) / UPS < up_ow;
            if (interior) {
                for (int e = threadIdx.x; e < C::GPIX * 6; e += 256) {
                    const int pix = e / 6, part = e - pix * 6;
                    const int r = pix >> 4, c = pix & 15;
                    f32x4 acc = zero4;
                    if constexpr (UPS == 1) {
                        const float *pb = s_up + ((r + 2) * UPW + (c + 2)) * UBD_C + 4 * part;      // patch pixel of tap (0, 0): row oy0 + up_pad + r - uy0 = r + 2
                        const float *wb = upk + 4 * part;
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                            for (int kx = 0; kx < 3; ++kx) {
                                const f32x4 v = *(const f32x4 *)(pb - (ky * UPW + kx) * UBD_C);
                                const f32x4 wv = *(const f32x4 *)(wb + (ky * 3 + kx) * UBD_C);
                                acc[0] = fmaf(v[0], wv[0], acc[0]); acc[1] = fmaf(v[1], wv[1], acc[1]);
                                acc[2] = fmaf(v[2], wv[2], acc[2]); acc[3] = fmaf(v[3], wv[3], acc[3]);
                            }
                    } else {
                        const int py = oy0 + r + up_pad, px = ox0 + c + up_pad;
                        const int qy = py & 1, qx = px & 1;
                        const float *pb = s_up + (((py >> 1) - uy0) * UPW + ((px >> 1) - ux0)) * UBD_C + 4 * part;   // tap (qy, qx)
                        const int t0 = qy * 3 + qx;
#pragma unroll
                        for (int a = 0; a < 2; ++a)
#pragma unroll
                            for (int b = 0; b < 2; ++b) {
                                const bool ok = (a == 0 || qy == 0) && (b == 0 || qx == 0);          // ky = qy + 2 a <= 2, kx = qx + 2 b <= 2
                                int t = t0 + 6 * a + 2 * b;
                                t = t > 8 ? 8 : t;
                                const f32x4 vl = *(const f32x4 *)(pb - (a * UPW + b) * UBD_C);
                                const f32x4 wv = *(const f32x4 *)(upk + t * UBD_C + 4 * part);
                                const f32x4 v = ok ? vl : zero4;
                                acc[0] = fmaf(v[0], wv[0], acc[0]); acc[1] = fmaf(v[1], wv[1], acc[1]);
                                acc[2] = fmaf(v[2], wv[2], acc[2]); acc[3] = fmaf(v[3], wv[3], acc[3]);
                            }
                    }
                    f32x4 *pg = (f32x4 *)(gtile + pix * C::GPIX_DW + 4 * part);
                    const f32x4 mk = *pg;
                    *pg = (f32x4){mk[0] > 0.f ? acc[0] : 0.f, mk[1] > 0.f ? acc[1] : 0.f, mk[2] > 0.f ? acc[2] : 0.f, mk[3] > 0.f ? acc[3] : 0.f};
                }
            } else
            for (int e = threadIdx.x; e < C::GPIX * 6; e += 256) {
                const int pix = e / 6, part = e - pix * 6;
                const int py = oy0 + (pix >> 4) + up_pad, px = ox0 + (pix & 15) + up_pad;
                f32x4 acc = zero4;
                // No branch around the two LDS reads of a tap (round 5: as `if (ok) { read; read; fma }` every tap was an LDS round trip of its
                // own): the patch index is clamped into the patch, a tap that does not exist contributes 0 * w (the same sum: x + 0 = x).
                // Stride 2: only taps of the pixel's parity can exist ((p - k) even), 2 x 2 of the 9 -- visited in the same ky, kx order.
                constexpr int NTAP = UPS == 1 ? 3 : 2;
#pragma unroll
                for (int a = 0; a < NTAP; ++a) {
                    const int ky = UPS == 1 ? a : (py & 1) + 2 * a;
                    const int ty = py - ky;
                    const bool yok = ky <= 2 && ty >= 0 && (ty / UPS) < up_oh;
                    int ur = (UPS == 1 ? ty : (ty >> 1)) - uy0;
                    ur = ur < 0 ? 0 : (ur > UPH - 1 ? UPH - 1 : ur);
#pragma unroll
                    for (int b = 0; b < NTAP; ++b) {
                        const int kx = UPS == 1 ? b : (px & 1) + 2 * b;
                        const int tx = px - kx;
                        const bool ok = yok && kx <= 2 && tx >= 0 && (tx / UPS) < up_ow;
                        int uc = (UPS == 1 ? tx : (tx >> 1)) - ux0;
                        uc = uc < 0 ? 0 : (uc > UPW - 1 ? UPW - 1 : uc);
                        int t = ky * 3 + kx;
                        t = t > 8 ? 8 : t;
                        const f32x4 vl = *(const f32x4 *)(s_up + (ur * UPW + uc) * UBD_C + 4 * part);
                        const f32x4 wv = *(const f32x4 *)(upk + t * UBD_C + 4 * part);
                        const f32x4 v = ok ? vl : zero4;
                        acc[0] = fmaf(v[0], wv[0], acc[0]); acc[1] = fmaf(v[1], wv[1], acc[1]);
                        acc[2] = fmaf(v[2], wv[2], acc[2]); acc[3] = fmaf(v[3], wv[3], acc[3]);
                    }
                }
                f32x4 *pg = (f32x4 *)(gtile + pix * C::GPIX_DW + 4 * part);
                const f32x4 mk = *pg;
                *pg = (f32x4){mk[0] > 0.f ? acc[0] : 0.f, mk[1] > 0.f ? acc[1] : 0.f, mk[2] > 0.f ? acc[2] : 0.f, mk[3] > 0.f ? acc[3] : 0.f};
            }
            SB32STAMP(7);
            __syncthreads();
        }
        SB32STAMP(8);
#pragma unroll 1
        for (int r = wid; r < C::TH; r += 4) {
            const int oy = oy0 + r;
            if (oy >= OH) break;
            const int ox = ox0 + i;
            const bool pvalid = ox < OW;
            // ---- 1. G of this pixel, channels 6q..6q+5 (zero outside the map: zero-fixed tile)
            float g6[6];
            {
                const f32x2 *pg = (const f32x2 *)(gtile + (r * 16 + i) * C::GPIX_DW + 6 * q);
                const f32x2 v0 = pg[0], v1 = pg[1], v2 = pg[2];
                g6[0] = v0[0]; g6[1] = v0[1]; g6[2] = v1[0]; g6[3] = v1[1]; g6[4] = v2[0]; g6[5] = v2[1];
            }
            // ---- 2. dDW[i][ch] = sum_co G[i][co] pw[ch][co]  (rows = channels in lane layout, cols = pixels)
            f32x4 dA = {0.f, 0.f, 0.f, 0.f}, dB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                dA = __builtin_amdgcn_mfma_f32_16x16x4f32(apw[s][0], g6[s], dA, 0, 0, 0);
                if constexpr (NT_A == 2) dB = __builtin_amdgcn_mfma_f32_16x16x4f32(apw[s][1], g6[s], dB, 0, 0, 0);
            }
            float ddwv[CPL];
            if constexpr (CIN == UBD_C) {
                ddwv[0] = dA[0]; ddwv[1] = dA[1]; ddwv[2] = dA[2]; ddwv[3] = dA[3]; ddwv[4] = dB[0]; ddwv[5] = dB[1];
            } else {
                ddwv[0] = dA[0];
            }
            // ---- 3. one pass over the taps: depthwise output (for dpw) and depthwise kernel gradient
            float dwv[CPL];
#pragma unroll
            for (int s = 0; s < CPL; ++s) dwv[s] = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int t = ky * 3 + kx;
                    const int pe = (CIN == UBD_C) ? (r * STRIDE + ky) * (C::XROW_DW * 4 / (int)sizeof(TX)) + C::xpos_dw(i * STRIDE + kx) * 4 / (int)sizeof(TX) + cb
                                                  : (r * STRIDE + ky) * C::XROW_E + xsk + (i * STRIDE + kx) * CIN + cb;     // element index (TX units)
                    const float *p = xpatch + pe;
                    if constexpr (CIN == UBD_C) {
                        float v[6];
                        ld_act6<TX>(xpatch, pe, v);
#pragma unroll
                        for (int s = 0; s < 6; ++s) { dwv[s] = fmaf(v[s], dwk[t][s], dwv[s]); ddw[t][s] = fmaf(v[s], ddwv[s], ddw[t][s]); }
                    } else {
                        dwv[0] = fmaf(p[0], dwk[t][0], dwv[0]);        // dwk is zero for lanes without a channel
                        ddw[t][0] = fmaf(ch_ok ? p[0] : 0.f, ddwv[0], ddw[t][0]);
                    }
                }
            // ---- 5. pointwise kernel / bias gradient: DW transposed through this wave's LDS tile, G read in place
#pragma unroll
            for (int s = 0; s < CPL; ++s)
                if (ch_ok) s_dw[wid][i][cb + s] = rnd_act<TR>(dwv[s]);
            __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's LDS writes have landed
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int pr = 4 * g4 + q;               // lane (m = i, k = q): pixel pr of this row tile
                const float *gp = gtile + (r * 16 + pr) * C::GPIX_DW;
                const float b0 = gp[i];
                const float b1 = i < 8 ? gp[16 + i] : 0.f;
                float a0, a1 = 0.f;
                if constexpr (CIN == UBD_C) {
                    a0 = s_dw[wid][pr][i];
                    a1 = i < 8 ? s_dw[wid][pr][16 + i] : (i == 8 ? 1.f : 0.f);
                } else {
                    a0 = i < CIN ? s_dw[wid][pr][i] : (i == CIN ? 1.f : 0.f);
                }
                accpw[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, accpw[0][0], 0, 0, 0);
                accpw[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, accpw[0][1], 0, 0, 0);
                if constexpr (MT_PW == 2) {
                    accpw[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, accpw[1][0], 0, 0, 0);
                    accpw[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, accpw[1][1], 0, 0, 0);
                }
            }
            __builtin_amdgcn_wave_barrier();
            // ---- 6. dDW for the data-gradient kernel
            if (dDW != nullptr && pvalid && ch_ok) {
                float *pd = dDW + (((size_t)img * OH + oy) * OW + ox) * CIN + cb;
                if constexpr (CIN == UBD_C) {
                    f32x2 *p2 = (f32x2 *)pd;
                    p2[0] = (f32x2){ddwv[0], ddwv[1]}; p2[1] = (f32x2){ddwv[2], ddwv[3]}; p2[2] = (f32x2){ddwv[4], ddwv[5]};
                } else {
                    pd[0] = ddwv[0];
                }
            }
        }
        SB32STAMP(9);
    }
    // ---- flush: block-level reduction in LDS, then this block's row of the partial-sum matrix
    //      row layout: [9*CIN depthwise | CIN*24 pointwise | 24 bias]
    constexpr int PART = 9 * CIN + CIN * UBD_C + UBD_C;
    __syncthreads();
    float *red = lds;                                   // tile buffers are free now
    for (int t = threadIdx.x; t < PART; t += blockDim.x) red[t] = 0.f;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s = 0; s < CPL; ++s) {
            float v = ddw[t][s];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            ddw[t][s] = v;
        }
    // the four waves add their sums one after the other (inside a wave every address has one writer): a fixed order -- the fp32 /
    // fp16 train step repeats bit for bit too since round 4 (LDS float atomics added the waves in whatever order they arrived)
    for (int ph = 0; ph < 4; ++ph) {
        if ((int)(threadIdx.x >> 6) == ph) {
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int s = 0; s < CPL; ++s)
                    if (i == 0 && ch_ok) red[t * CIN + cb + s] += ddw[t][s];
            // pointwise kernel / bias gradient: D col = i (co), row = 4q + r (+16 mt) (ci or the ones row)
#pragma unroll
            for (int mt = 0; mt < MT_PW; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * mt + 4 * q + r, col = i + 16 * nt;
                        if (col < UBD_C && row <= CIN) red[9 * CIN + row * UBD_C + col] += accpw[mt][nt][r];   // row CIN = bias
                    }
        }
        __syncthreads();
    }
    float *prow = partials + (size_t)blockIdx.x * PART;
    for (int t = threadIdx.x; t < PART; t += blockDim.x) prow[t] = red[t];
}

// G_below[q][c] = (sum_t dDW[(q + pad - t)/s][c] dw[t][c]) * (X[q][c] > 0)   (24-channel layers only)
template <int STRIDE, typename TX>
__global__ __launch_bounds__(256) void sep_dx_kernel(const float *__restrict__ dDW, const void *__restrict__ xmask,
                                                     float *__restrict__ gout, const float *__restrict__ fwdfrag, int n, int H,
                                                     int W, int OH, int OW, int pad_lo)
{
    const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
    const float *dwlane = fwdfrag + UBD_SEP_FRAG_FLOATS;
    float dwk[9][6];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s = 0; s < 6; ++s) dwk[t][s] = rnd_act<TX>(dwlane[(t * 6 + s) * 64 + lane]);
    const int tiles_x = (W + 15) >> 4;
    const int total = n * H * tiles_x;
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < total; tile += nwaves) {
        const int xt = (int)((unsigned)tile % (unsigned)tiles_x);
        const int rowid = (int)((unsigned)tile / (unsigned)tiles_x);
        const int iy = (int)((unsigned)rowid % (unsigned)H);
        const int img = (int)((unsigned)rowid / (unsigned)H);
        const int ix = xt * 16 + i;
        if (ix >= W) continue;
        float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = iy - ky + pad_lo;
            const bool yok = ty >= 0 && (STRIDE == 1 || (ty & 1) == 0) && (ty / STRIDE) < OH;
            const int oy = ty / STRIDE;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = ix - kx + pad_lo;
                const bool ok = yok && tx >= 0 && (STRIDE == 1 || (tx & 1) == 0) && (tx / STRIDE) < OW;
                if (ok) {
                    const int ox = tx / STRIDE;
                    const f32x2 *p = (const f32x2 *)(dDW + (((size_t)img * OH + oy) * OW + ox) * UBD_C + 6 * q);
                    const f32x2 v0 = p[0], v1 = p[1], v2 = p[2];
                    const int t = ky * 3 + kx;
                    acc[0] = fmaf(v0[0], dwk[t][0], acc[0]); acc[1] = fmaf(v0[1], dwk[t][1], acc[1]);
                    acc[2] = fmaf(v1[0], dwk[t][2], acc[2]); acc[3] = fmaf(v1[1], dwk[t][3], acc[3]);
                    acc[4] = fmaf(v2[0], dwk[t][4], acc[4]); acc[5] = fmaf(v2[1], dwk[t][5], acc[5]);
                }
            }
        }
        const size_t e = (((size_t)img * H + iy) * W + ix) * UBD_C + 6 * q;
        float mk[6];
        ld_act6<TX>(xmask, e, mk);
        f32x2 *po = (f32x2 *)(gout + e);
        po[0] = (f32x2){mk[0] > 0.f ? acc[0] : 0.f, mk[1] > 0.f ? acc[1] : 0.f};
        po[1] = (f32x2){mk[2] > 0.f ? acc[2] : 0.f, mk[3] > 0.f ? acc[3] : 0.f};
        po[2] = (f32x2){mk[4] > 0.f ? acc[4] : 0.f, mk[5] > 0.f ? acc[5] : 0.f};
    }
}

// UPS > 0: G is computed in the kernel from the layer above (G = this layer's output activation, the mask source; up_*: see the kernel)
template <int CIN, int STRIDE, typename TX, typename TR = TX, int UPS = 0>
static int launch_sep_bwd(const ubd_handle *h, const void *x, int in_u8, const float *G, float *dDW, const float *ffrag,
                           const float *bfrag, float *grads, int s, rp_queue *rq, int n, int H, int W,
                           int OH, int OW, int pad_lo, float sub, float div, hipStream_t st,
                           const float *up_ddw = nullptr, const float *up_dw = nullptr, int up_oh = 0, int up_ow = 0, int up_pad = 0)
{
    using C = sepb_cfg<CIN, STRIDE, (int)sizeof(TX), UPS>;
    // the kernel addresses a tile's pieces as image base + 32-bit byte offset
    if ((CIN == UBD_C && (unsigned long long)H * W * UBD_C * sizeof(TX) > 0xFFFFFFFFull) || (unsigned long long)OH * OW * UBD_C * 4 > 0xFFFFFFFFull) {
        ubd_set_error("separable backward: one image's activation map exceeds 4 GiB (%d x %d)", H, W);
        return -1;
    }
    if (UPS > 0 && (unsigned long long)up_oh * up_ow * UBD_C * 4 > 0xFFFFFFFFull) { ubd_set_error("separable backward: upper map exceeds 4 GiB"); return -1; }
    const int th = C::TH;
    const long tiles = (long)n * ((OH + th - 1) / th) * ((OW + 15) / 16);
    const size_t up_bytes = UPS == 0 ? 16 : ((UPS == 1 ? (size_t)(th + 2) * 18 : (size_t)(th / 2 + 2) * 10) * UBD_C + 9 * UBD_C) * sizeof(float);
    const size_t lds_bytes = C::LDS_FLOATS * sizeof(float) + 4 * 16 * (CIN == UBD_C ? UBD_C : 4) * sizeof(float) + up_bytes;
    int grid = h->num_cus * (lds_bytes > 80 * 1024 ? 1 : (lds_bytes > 53 * 1024 ? 2 : (lds_bytes > 40 * 1024 || !(CIN != UBD_C && UPS > 0) ? 3 : 4)));   // 160 KB of LDS per CU
    if (grid > tiles) grid = (int)tiles;
    const int part = 9 * CIN + CIN * UBD_C + UBD_C;
    float *partials = rp_add(rq, grid, part, grads + h->off_sep_dw[s], 9 * CIN, grads + h->off_sep_pw[s], CIN * UBD_C, grads + h->off_sep_b[s], st);
    if (!partials) return -1;
    auto launch = [&](auto u8) {
        hipLaunchKernelGGL((sep_bwd_kernel<CIN, STRIDE, decltype(u8)::value, TX, TR, UPS>), dim3(grid), dim3(256), 0, st, x, G, dDW, ffrag, bfrag, partials, n, H, W, OH, OW, pad_lo, sub, div, up_ddw, up_dw, up_oh, up_ow, up_pad UBD_STAMP_ARG("sep_bwd", CIN, STRIDE));
    };
    in_u8 ? launch(int_c<1>()) : launch(int_c<0>());
    return 0;
}

// fp32 gradient tensors between the layers: fp32 and fp16 activations (16-bit gradient tensors would underflow in fp16 without loss
// scaling).  Head and dilated layers here, the separable layers in sep_backward_f32.
template <typename TX>
int bwd_pass::backward_f32()
{
    const int H4 = H / 4, W4 = W / 4;
    const long npix = (long)n * H4 * W4;
    float *bfrag = (float *)(ws + T.off_bfrag);
    UBD_CHECK_HIP(hipMemsetAsync(grads, 0, h->n_params * sizeof(float), st));
    hipLaunchKernelGGL(pack_bwd_kernel, dim3(64), dim3(256), 0, st, params, bfrag, fill_pack_args(h).pb);
    if (h->use_wino) ubd_launch_pack_wino(h, params, bfrag + UBD_BWD_DIRECT_FLOATS, 1, st);

    float *gq[2] = {(float *)(ws + T.off_gq[0]), (float *)(ws + T.off_gq[1])};
    rp_queue rq;
    rp_init(&rq, (float *)(ws + T.off_partials), T.partials_floats);
    const int grid = (int)std::min<long>((npix + 255) / 256, h->num_cus * 8);
    int cur = 0;
    // head
    hipLaunchKernelGGL((head_dx_kernel<TX>), dim3(grid), dim3(256), 0, st, dlogits, acts[6], params + h->off_head_k, gq[0], npix, h->k_out);
    if (launch_head_wgrad<TX>(h, acts[6], dlogits, grads, &rq, npix, st)) return -1;
    // dilated layers, top to bottom
    for (int k = UBD_NUM_DIL - 1; k >= 0; --k) {
        const void *X = acts[k];                                // input of dilated layer k (= output of the layer below)
        const int dd = UBD_DILATIONS[k];
        const long items = (long)n * dd * dd * (((H4 + dd - 1) / dd + WG_TH - 1) / WG_TH) * (((W4 + dd - 1) / dd + WG_TW - 1) / WG_TW);
        int gw = (int)std::min<long>(items, h->num_cus * 2);
        gw = (gw + 7) / 8 * 8;                                  // the item ranges are cut per XCD: all eight need a block
        float *partials = rp_add(&rq, gw, 217 * UBD_C, grads + h->off_dil_k[k], 216 * UBD_C, grads + h->off_dil_b[k], UBD_C, nullptr, st);
        if (!partials) return -1;
        if constexpr (sizeof(TX) == 4) {
            if (h->split_sepbwd32) hipLaunchKernelGGL((dil_wgrad_kernel<TX>), dim3(gw), dim3(256), 0, st, X, gq[cur], partials, n, H4, W4, dd);     // diagnostics: the four-wave form
            else hipLaunchKernelGGL((dil_wgrad_kernel<TX, 2>), dim3(gw), dim3(512), 0, st, X, gq[cur], partials, n, H4, W4, dd);
        } else
            hipLaunchKernelGGL((dil_wgrad_kernel<TX>), dim3(gw), dim3(256), 0, st, X, gq[cur], partials, n, H4, W4, dd);
        if (h->use_wino)
            ubd_launch_dilconv_wino(h, 1, bfrag + UBD_BWD_DIRECT_FLOATS + (size_t)k * UBD_WINO_FRAG_FLOATS, X, h->cfg.dtype, dd, gq[cur], gq[cur ^ 1], n, H4, W4, st);
        else
            ubd_launch_dilconv(h, 1, bfrag + (size_t)k * UBD_DIL_FRAG_FLOATS, (const float *)X, dd, gq[cur], gq[cur ^ 1], n, H4, W4, st);
        cur ^= 1;
    }
    rp_flush(&rq, st);
    if (ubd_comm_fused(h)) { const int rc = ubd_comm_begin_tail(h, grads, st); if (rc) return rc; }       // dilated + head gradients are final
    return sep_backward_f32<TX>(gq[cur], &rq);
}

// separable layers L3, L2, L1 of that pass; G3: the gradient at L3's output
template <typename TX>
int bwd_pass::sep_backward_f32(const float *G3, rp_queue *rq)
{
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
    float *ddw3 = (float *)(ws + T.off_ddw3), *gb[2] = {(float *)(ws + T.off_gb[0]), (float *)(ws + T.off_gb[1])};
    const int pad_s2 = h->cfg.fml_compatible ? 1 : 0;
    const int per_sep = UBD_SEP_FRAG_FLOATS + UBD_SEP_DW_FLOATS;
    const float *sf0 = wfrag, *sf1 = wfrag + per_sep, *sf2 = wfrag + 2 * per_sep;
    const float *bs0 = (const float *)(ws + T.off_bfrag) + UBD_BWD_DGRAD_FLOATS, *bs1 = bs0 + UBD_BWD_SEP_FLOATS, *bs2 = bs1 + UBD_BWD_SEP_FLOATS;
    const input_affine_t in = input_affine(preprocessing, in_dtype);
    // L3: input a2 (H2 x W2), output H4 x W4
    if (launch_sep_bwd<UBD_C, 2, TX>(h, a2, 0, G3, ddw3, sf2, bs2, grads, 2, rq, n, H2, W2, H4, W4, pad_s2, 0.f, 1.f, st)) return -1;
    if constexpr (sizeof(TX) == 4) {
        // fp32 activations: L2's and L1's kernels build their G tiles themselves from the dDW tensor of the layer above and their own
        // output activation (the ReLU mask) -- no sep_dx launches, no G tensors (UBD_SEPBWD=split keeps the two-kernel form)
        if (!h->split_sepbwd32) {
            const float *dwk2 = params + h->off_sep_dw[2], *dwk1 = params + h->off_sep_dw[1];
            if (launch_sep_bwd<UBD_C, 1, TX, TX, 2>(h, a1, 0, (const float *)a2, gb[1], sf1, bs1, grads, 1, rq, n, H2, W2, H2, W2, 1, 0.f, 1.f, st,
                                                    ddw3, dwk2, H4, W4, pad_s2)) return -1;
            if (with_c_in(h, [&](auto c) {
                    return launch_sep_bwd<decltype(c)::value, 2, float, TX, 1>(h, images, in.u8, (const float *)a1, nullptr, sf0, bs0, grads, 0, rq, n, H, W, H2, W2,
                                                                                pad_s2, in.sub, in.div, st, gb[1], dwk1, H2, W2, 1);
                })) return -1;
            return finish_step(h, rq, grads, st);
        }
    }
    const int g3 = ubd_grid_for((long)n * H2 * ((W2 + 15) / 16), h->num_cus, 4, 8);
    hipLaunchKernelGGL((sep_dx_kernel<2, TX>), dim3(g3), dim3(256), 0, st, ddw3, a2, gb[0], sf2, n, H2, W2, H4, W4, pad_s2);
    // L2: input a1, output H2 x W2, G = gb[0]
    if (launch_sep_bwd<UBD_C, 1, TX>(h, a1, 0, gb[0], gb[1], sf1, bs1, grads, 1, rq, n, H2, W2, H2, W2, 1, 0.f, 1.f, st)) return -1;
    hipLaunchKernelGGL((sep_dx_kernel<1, TX>), dim3(g3), dim3(256), 0, st, gb[1], a1, gb[0], sf1, n, H2, W2, H2, W2, 1);
    // L1: input = images (fp32 / uint8), no data gradient
    if (with_c_in(h, [&](auto c) {
            return launch_sep_bwd<decltype(c)::value, 2, float, TX>(h, images, in.u8, gb[0], nullptr, sf0, bs0, grads, 0, rq, n, H, W, H2, W2, pad_s2, in.sub, in.div, st);
        })) return -1;
    return finish_step(h, rq, grads, st);
}
template int bwd_pass::backward_f32<float>();
template int bwd_pass::backward_f32<_Float16>();
