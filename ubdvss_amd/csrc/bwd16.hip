// Backward pass of the UBD_BF16 train step, with bf16 gradient tensors between the layers (bwd_pass::backward_bf16): the kernels are in
// bwd16.h (head, dilated layers) and sepbwd16.h (separable layers); the step's one-launch prologue.
#include "bwd16.h"
#include "sepbwd16.h"

template <int CIN, int STRIDE, int GSRC, typename T>
static int launch_sepb16(const ubd_handle *h, const void *x, int in_u8, const unsigned short *D, const unsigned *mbits, unsigned *xbits,
                          unsigned short *dDW, const float *dw_own, const float *pw_own, const float *dw_up, float *grads, int s,
                          rp_queue *rq, int n, int H, int W, int OH, int OW, int pad_lo, int DH, int DWd, int pad_up,
                          float sub, float div, hipStream_t st)
{
    using C = sepb16_cfg<CIN, STRIDE, GSRC>;
    // 1/3-channel fp32 input that is already preprocessed, rows a whole number of 16-byte chunks: the patch is fetched by LDS-DMA
    // (UBD_SEPB16_X=regs keeps the register path, which also serves every other input)
    bool xdma = false;
    if constexpr (CIN != UBD_C)
        xdma = !in_u8 && sub == 0.f && div == 1.f && (W * CIN) % 4 == 0 && ((uintptr_t)x & 15) == 0 && (unsigned)pad_lo <= 1u && !h->sepb_x_regs &&
               (size_t)H * W * CIN * 4 < (1ull << 31);      // the kernel's 'outside the image' offset 0x80000000 must lie beyond one image's bytes (the register path serves larger images)
    const long tiles = (long)n * ((OH + C::TH - 1) / C::TH) * ((OW + 15) / 16);
    int grid = h->num_cus * (xdma ? sepb16_cfg<CIN, STRIDE, GSRC, 1>::BLOCKS_PER_CU : C::BLOCKS_PER_CU);
    if (grid > tiles) grid = (int)tiles;
    const rp_job prev = h->chain_reduce ? rp_take_prev(rq) : rp_job{};
    float *partials = rp_add(rq, grid, C::PART, grads + h->off_sep_dw[s], 9 * CIN, grads + h->off_sep_pw[s], CIN * UBD_C, grads + h->off_sep_b[s], st);
    if (!partials) return -1;
    auto launch = [&](auto xb) {      // 0: fp32 input through registers, 1: uint8, 2: fp32 by LDS-DMA
        hipLaunchKernelGGL((sepb16_kernel<CIN, STRIDE, decltype(xb)::value, GSRC, T>), dim3(grid), dim3(C::NT), 0, st, x, D, mbits, xbits, dDW, dw_own, pw_own, dw_up, partials, n, H, W, OH, OW, pad_lo, DH, DWd, pad_up, sub, div, prev UBD_STAMP_ARG("sepb16", CIN, STRIDE));
    };
    if constexpr (CIN != UBD_C) {
        if (xdma) { launch(int_c<2>()); return 0; }
    }
    in_u8 ? launch(int_c<1>()) : launch(int_c<0>());
    return 0;
}

// Weight gradient of a bf16 dilated layer and, with fuse_dx, its data gradient from the same staged tiles (bwd16.h).  tw: tile width;
// pair: two 8-wide sub-grids side by side in one 16-wide tile (bwd16.h PAIR).  8-wide tiles take the M-split accumulators in both forms.
template <typename TX>
static void launch_dil_wgrad16(int gw, const void *X, const unsigned short *G, float *partials, int n, int H4, int W4, int dd,
                               const unsigned *wt, unsigned short *g_out, const rp_job &prev, int tw, bool pair, bool fuse_dx, hipStream_t st)
{
    auto launch = [&](auto tw_c, auto dx_c, auto pair_c) {
        constexpr int TW = decltype(tw_c)::value;
        constexpr bool DX = decltype(dx_c)::value, PAIR = decltype(pair_c)::value;
        hipLaunchKernelGGL((dil_wgrad16_kernel<TX, TW, DX, TW == 8, PAIR>), dim3(gw), dim3(256), 0, st, (const unsigned short *)X, G, partials, n, H4, W4, dd,
                           DX ? (const u32x4 *)wt : nullptr, DX ? g_out : nullptr, prev, w16_geometry<TW, PAIR>(n, H4, W4, dd) UBD_STAMP_ARG("dil_wgrad16", dd));
    };
    if (pair) launch(int_c<16>(), std::true_type(), std::true_type());
    else if (tw == 8 && fuse_dx) launch(int_c<8>(), std::true_type(), std::false_type());
    else if (tw == 8) launch(int_c<8>(), std::false_type(), std::false_type());
    else if (fuse_dx) launch(int_c<16>(), std::true_type(), std::false_type());
    else launch(int_c<16>(), std::false_type(), std::false_type());
}

// One launch in front of the bf16 train step: the four weight packers (fp32 stem fragments, 16-bit dilated fragments, backward
// fragments, transposed 16-bit fragments: 48 blocks each) + zero gradient vector + zero loss scratch -- they were four ~5-us
// kernels and two memset kernels scattered over the step, each serialised behind its predecessor (rocprofv3: 29 us of a 1.22-ms step).
template <typename T>
__global__ __launch_bounds__(256) void train_prologue16_kernel(const float *__restrict__ params, train_prologue_args a)
{
    const int part = (int)blockIdx.x / 48, vtid = ((int)blockIdx.x % 48) * 256 + (int)threadIdx.x, vthreads = 48 * 256;
    if (part == 0) pack_weights_body(params, a.wfrag32, a.pa, vtid, vthreads);
    else if (part == 1) {
        pack16_body<T>(params, a.wfrag16, a.off0, a.layer_stride, 0, vtid, vthreads);
        pack_sep16_ready_body<T>(params, a.wfrag16 + UBD_NUM_DIL * UBD_DIL16_FRAG_U32, a.ps, vtid, vthreads);
    }
    else if (part == 2) pack_bwd_body(params, a.bfrag, a.pb, vtid, vthreads);
    else pack16_body<T>(params, a.frag16t, a.off0, a.layer_stride, 1, vtid, vthreads);
    const size_t gtid = (size_t)blockIdx.x * 256 + threadIdx.x, gthreads = (size_t)gridDim.x * 256;
    for (size_t i = gtid; i < a.n_params; i += gthreads) a.grads[i] = 0.f;
    for (size_t i = gtid; i < a.loss_zero_words; i += gthreads) a.loss_zero[i] = 0u;
}

void bwd_pass::prologue_bf16()
{
    train_prologue_args a = fill_pack_args(h);
    a.loss_zero_words = ubd_loss_zero_bytes() / 4;
    a.wfrag32 = (float *)(ws + T.fwd16.off_wfrag32); a.wfrag16 = (unsigned *)(ws + T.fwd16.off_wfrag16);
    a.bfrag = (float *)(ws + T.off_bfrag); a.frag16t = (unsigned *)(a.bfrag + UBD_BWD_DIRECT_FLOATS);
    a.grads = grads; a.loss_zero = (unsigned *)(ws + T.off_loss);
    hipLaunchKernelGGL((train_prologue16_kernel<__bf16>), dim3(4 * 48), dim3(256), 0, st, params, a);
}

// The bf16 step, with bf16 gradient tensors (bwd16.h, sepbwd16.h): G9..G3 live in the two halves of gq[0].  The step's prologue kernel
// has zeroed the gradient vector and packed every fragment; the transposed 16-bit fragments take the Winograd part of bfrag.
int bwd_pass::backward_bf16()
{
    using TX = __bf16;
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
    const long npix = (long)n * H4 * W4;
    const unsigned *frag16t = (const unsigned *)((const float *)(ws + T.off_bfrag) + UBD_BWD_DIRECT_FLOATS);
    unsigned short *g16[2] = {(unsigned short *)(ws + T.off_gq[0]), (unsigned short *)(ws + T.off_gq[0]) + (size_t)npix * UBD_C};
    const unsigned short *a9 = (const unsigned short *)acts[6];
    rp_queue rq;
    rp_init(&rq, (float *)(ws + T.off_partials), T.partials_floats);
    int cur = 0;
    if (h->k_out == 1) {                                       // one pass over A9 for both head gradients
        int g1 = (int)std::min<long>((npix * 3 + 255) / 256, h->num_cus * 6);
        g1 = (g1 + 2) / 3 * 3;                                 // 256 g1 = 0 (mod 3): a thread keeps its channel group
        float *partials = rp_add(&rq, g1, UBD_C + 1, grads + h->off_head_k, UBD_C, grads + h->off_head_b, 1, nullptr, st);
        if (!partials) return -1;
        hipLaunchKernelGGL((head_bwd1_16_kernel<TX>), dim3(g1), dim3(256), 0, st, dlogits, a9, params + h->off_head_k, g16[0], partials, npix);
    } else if (h->split_headbwd) {                            // UBD_HEADBWD=split: the two kernels
        const int grid = (int)std::min<long>((npix + 255) / 256, h->num_cus * 8);
        hipLaunchKernelGGL((head_dx16_kernel<TX>), dim3(grid), dim3(256), 0, st, dlogits, a9, params + h->off_head_k, g16[0], npix, h->k_out);
        if (launch_head_wgrad<TX>(h, a9, dlogits, grads, &rq, npix, st)) return -1;
    } else if (launch_head_wgrad<TX, true>(h, a9, dlogits, grads, &rq, npix, st, params + h->off_head_k, g16[0])) return -1;
    for (int k = UBD_NUM_DIL - 1; k >= 0; --k) {
        const void *X = acts[k];
        const int dd = UBD_DILATIONS[k];
        const int sw = (W4 + dd - 1) / dd, tw = sw <= 8 ? 8 : 16;              // narrow sub-grids: 8-wide tiles
        // sub-grids exactly 8 columns wide and at most 8 rows high (dilation 16 on 128 x 128 maps): two of them side by side in one 16-wide tile
        // (UBD_DILBWD=pair8 keeps the 8-wide form)
        const bool pair = !h->split_dilbwd && !h->no_pair_dilbwd && tw == 8 && sw == 8 && (dd & 1) == 0 && W4 % dd == 0 && (H4 + dd - 1) / dd <= 8;
        const long items = pair ? (long)n * dd * (dd / 2)
                                : (long)n * dd * dd * (((H4 + dd - 1) / dd + W16_TH(tw) - 1) / W16_TH(tw)) * ((sw + tw - 1) / tw);
        int gw = (int)std::min<long>(items, h->num_cus * ((tw == 8 && !pair) ? 3 : 2));     // 16 x 16 tiles: two blocks per CU (LDS, registers); 8-wide tiles: three; the same grid in the split mode (same order of the partial sums)
        gw = (gw + 7) / 8 * 8;                                  // the item ranges are cut per XCD: all eight need a block
        const rp_job prev = h->chain_reduce ? rp_take_prev(&rq) : rp_job{};   // the head's / the layer above's partial rows: totalled at the end of this kernel
        float *partials = rp_add(&rq, gw, 217 * UBD_C, grads + h->off_dil_k[k], 216 * UBD_C, grads + h->off_dil_b[k], UBD_C, nullptr, st);
        if (!partials) return -1;
        const unsigned *wt = frag16t + (size_t)k * UBD_DIL16_FRAG_U32;
        const bool fuse_dx = !h->split_dilbwd;                  // UBD_DILBWD=split keeps the separate data-gradient kernel
        launch_dil_wgrad16<TX>(gw, X, g16[cur], partials, n, H4, W4, dd, wt, g16[cur ^ 1], prev, tw, pair, fuse_dx, st);
        if (!fuse_dx) ubd_launch_dilconv16(h, 1, wt, nullptr, X, dd, g16[cur], g16[cur ^ 1], n, H4, W4, st);
        cur ^= 1;
    }
    // chained reduction: the first dilated layer's rows are totalled at the end of L3's kernel below, so the dilated + head segment
    // is final (and its all-reduce may start) one kernel later than with the stand-alone reduction
    if (!h->chain_reduce) {
        rp_flush(&rq, st);
        if (ubd_comm_fused(h)) { const int rc = ubd_comm_begin_tail(h, grads, st); if (rc) return rc; }   // dilated + head gradients are final
    }
    // separable layers: G1 / G2 are built tile-wise in LDS from the bf16 dDW tensor of the layer above (sepbwd16.h)
    const int pad2 = h->cfg.fml_compatible ? 1 : 0;
    const float *dw0 = params + h->off_sep_dw[0], *dw1 = params + h->off_sep_dw[1], *dw2 = params + h->off_sep_dw[2];
    const float *pw0 = params + h->off_sep_pw[0], *pw1 = params + h->off_sep_pw[1], *pw2 = params + h->off_sep_pw[2];
    unsigned short *ddw3 = (unsigned short *)(ws + T.off_ddw3), *ddw2 = (unsigned short *)(ws + T.off_gb[0]);
    // ReLU bits of a2 and a1 (one word per pixel, sepbwd16.h): written by the kernel that reads the activation as its input, read by the next one
    unsigned *bits2 = (unsigned *)(ws + T.off_gb[1]), *bits1 = bits2 + ubd_align_up((size_t)n * H2 * W2, 64);
    if (launch_sepb16<UBD_C, 2, 0, TX>(h, a2, 0, g16[cur], nullptr, bits2, ddw3, dw2, pw2, dw2, grads, 2, &rq, n, H2, W2, H4, W4, pad2, H4, W4, 0, 0.f, 1.f, st)) return -1;
    if (h->chain_reduce && ubd_comm_fused(h)) { const int rc = ubd_comm_begin_tail(h, grads, st); if (rc) return rc; }   // dilated + head gradients are final
    if (launch_sepb16<UBD_C, 1, 2, TX>(h, a1, 0, ddw3, bits2, bits1, ddw2, dw1, pw1, dw2, grads, 1, &rq, n, H2, W2, H2, W2, 1, H4, W4, pad2, 0.f, 1.f, st)) return -1;
    const input_affine_t in = input_affine(preprocessing, in_dtype);
    if (with_c_in(h, [&](auto c) {
            return launch_sepb16<decltype(c)::value, 2, 1, TX>(h, images, in.u8, ddw2, bits1, nullptr, nullptr, dw0, pw0, dw1, grads, 0, &rq, n, H, W, H2, W2, pad2, H2, W2, 1, in.sub, in.div, st);
        })) return -1;
    return finish_step(h, &rq, grads, st);
}
