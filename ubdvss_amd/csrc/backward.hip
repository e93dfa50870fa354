// Train-step orchestration of the ubdvss hot path on gfx950: the workspace layout, ubd_train_step (and the two halves of a step that
// the multi-scale step runs per level), and the stand-alone reduction of the weight gradients' partial sums.
//
// The reference gets its gradients from TensorFlow autodiff of the Keras graph
// (model.compile / fit_generator, train.py:110-112, :176-188); here every gradient kernel is
// written out, in one of two backward passes: bwd32.hip (fp32 and fp16 activations, fp32 gradient tensors) and bwd16.hip (bf16).
// Weight gradients: every block writes one row of a partial-sum matrix, reduce_partials_kernel adds the rows in a
// fixed order into the flat gradient vector (Keras get_weights() order, same as the parameters).
#include "bwd_common.h"

__global__ __launch_bounds__(256) void reduce_partials_kernel(const rp_batch B)
{
    int j = 0;
#pragma unroll
    for (int k = 1; k < RP_MAX_JOBS; ++k)
        if (k < B.njobs && (int)blockIdx.x >= B.job[k].block0) j = k;            // block-uniform
    // block = RP_COLS consecutive elements x (256 / RP_COLS) row groups.
    // 16 columns per block: 5208-element rows give 326 blocks (one per CU and more) instead of 82.
    __shared__ float s[256];
    rp_reduce_group(B.job[j], (int)blockIdx.x - B.job[j].block0, s);
}

// Host side of the batched reduction (bwd_common.h)
void rp_init(rp_queue *q, float *base, size_t cap_floats) { q->b.njobs = 0; q->nblocks = 0; q->base = base; q->used = 0; q->cap = cap_floats; }
rp_job rp_take_prev(rp_queue *q)
{
    rp_job j;
    memset(&j, 0, sizeof(j));
    if (q->b.njobs > 0) {
        j = q->b.job[--q->b.njobs];
        q->nblocks = j.block0;
        j.block0 = 0;
    }
    return j;
}
int rp_flush(rp_queue *q, hipStream_t st)
{
    if (q->b.njobs > 0) hipLaunchKernelGGL(reduce_partials_kernel, dim3(q->nblocks), dim3(256), 0, st, q->b);
    q->b.njobs = 0; q->nblocks = 0;                            // the matrices stay allocated until the pass ends (the kernel is in flight)
    return 0;
}
float *rp_add(rp_queue *q, int rows, int count, float *out0, int n0, float *out1, int n1, float *out2, hipStream_t st)
{
    if (q->b.njobs == RP_MAX_JOBS) rp_flush(q, st);
    const size_t need = ((size_t)rows * count + 63) & ~(size_t)63;
    if (q->used + need > q->cap) { ubd_set_error("backward: partial-sum region too small (%zu + %zu > %zu floats)", q->used, need, q->cap); return nullptr; }
    float *part = q->base + q->used;
    q->used += need;
    rp_job &j = q->b.job[q->b.njobs++];
    j.part = part; j.out0 = out0; j.out1 = out1; j.out2 = out2; j.nblocks = rows; j.count = count; j.n0 = n0; j.n1 = n1; j.block0 = q->nblocks;
    q->nblocks += (count + RP_COLS - 1) / RP_COLS;
    return part;
}

void ubd_train_layout_compute(const ubd_handle *h, int n, int H, int W, train_layout *T)
{
    size_t off;
    if (h->cfg.dtype == UBD_F32) { ubd_fwd_layout_compute(h, n, H, W, 1, &T->fwd); off = T->fwd.total; }
    else { ubd_fwd16_layout_compute(n, H, W, 1, &T->fwd16); off = T->fwd16.total; }
    const size_t small = ubd_align_up((size_t)n * (H / 4) * (W / 4) * UBD_C * sizeof(float), 256);
    const size_t big = ubd_align_up((size_t)n * (H / 2) * (W / 2) * UBD_C * sizeof(float), 256);
    const size_t lg = ubd_align_up((size_t)n * (H / 4) * (W / 4) * h->k_out * sizeof(float), 256);
    T->off_bfrag = off;   off += ubd_align_up(UBD_BWD_FRAG_FLOATS * sizeof(float), 256);
    T->off_logits = off;  off += lg;
    T->off_dlogits = off; off += lg;
    T->off_gq[0] = off;   off += small;
    T->off_gq[1] = off;   off += small;
    T->off_ddw3 = off;    off += small;
    T->off_gb[0] = off;   off += big;
    T->off_gb[1] = off;   off += big;
    T->off_loss = off;    off += ubd_align_up(ubd_loss_workspace_bytes(h, n, H / 4, W / 4), 256);
    T->partials_floats = (size_t)8 * ((size_t)4 * h->num_cus + 8) * (217 * UBD_C);      // one matrix per producer (ten per pass), freed at the end of the pass
    T->off_partials = off; off += ubd_align_up(T->partials_floats * sizeof(float), 256);
    T->total = off;
}

extern "C" size_t ubd_train_workspace_bytes(const ubd_handle *h, int n, int height, int width)
{
    if (!h) return 0;
    train_layout T;
    ubd_train_layout_compute(h, n, height, width, &T);
    return T.total;
}

// The forward half of a step over p's workspace, keeping every activation: on bf16 handles the one-launch prologue first, then the
// handle's training forward into `logits`; fills in what the backward pass reads of it.  ubd_train_step and every level of
// ubd_train_step_multiscale (multiscale.hip) run this and ubd_train_backward.
int ubd_train_forward(bwd_pass &p, float *logits)
{
    ubd_handle *h = p.h;
    char *ws = p.ws;
    const train_layout &T = p.T;
    const bool f32 = h->cfg.dtype == UBD_F32, bf16 = h->cfg.dtype == UBD_BF16;
    int rc;
    if (f32) {
        rc = ubd_forward_impl(h, p.params, p.images, p.in_dtype, p.preprocessing, p.n, p.H, p.W, logits, ws, T.fwd, p.st);
        p.a1 = ws + T.fwd.off_a1; p.a2 = ws + T.fwd.off_a2; p.wfrag = (const float *)(ws + T.fwd.off_wfrag);
        for (int k = 0; k < 7; ++k) p.acts[k] = ws + T.fwd.off_acts[k];
    } else {
        UBD_REQUIRE(p.in_dtype == UBD_IN_F32 || p.in_dtype == UBD_IN_U8, "ubd_train_step: bad in_dtype %d", p.in_dtype);
        if (bf16) p.prologue_bf16();                               // the one-launch prologue: everything packed, gradients and loss scratch zeroed
        rc = ubd_forward16_layout(h, p.params, p.images, bf16 ? (p.in_dtype | UBD_IN_PREPACKED) : p.in_dtype, p.preprocessing, p.n, p.H, p.W, logits, ws, T.fwd16, p.st);
        p.a1 = ws + T.fwd16.off_a1; p.a2 = ws + T.fwd16.off_a2; p.wfrag = (const float *)(ws + T.fwd16.off_wfrag32);
        for (int k = 0; k < 7; ++k) p.acts[k] = ws + T.fwd16.off_acts[k];
    }
    return rc;
}

int ubd_train_backward(bwd_pass &p)
{
    const int dt = p.h->cfg.dtype;
    return dt == UBD_BF16 ? p.backward_bf16() : dt == UBD_F32 ? p.backward_f32<float>() : p.backward_f32<_Float16>();
}

extern "C" int ubd_train_step(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                              const int32_t *y_true, int n, int height, int width, float *grads, float *loss,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    UBD_REQUIRE(h && params && images && y_true && grads && loss && workspace, "ubd_train_step: null argument");
    UBD_REQUIRE(n > 0 && height > 0 && width > 0 && (height % 4) == 0 && (width % 4) == 0, "ubd_train_step: height and width must be positive multiples of 4");
    UBD_REQUIRE(h->cfg.dtype == UBD_F32 || h->use_wino, "ubd_train_step: 16-bit activations need the Winograd data-gradient kernel (unset UBD_DILCONV=direct)");
    train_layout T;
    ubd_train_layout_compute(h, n, height, width, &T);
    UBD_REQUIRE(workspace_bytes >= T.total, "ubd_train_step: workspace too small (%zu < %zu)", workspace_bytes, T.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *logits = (float *)(ws + T.off_logits), *dlogits = (float *)(ws + T.off_dlogits);
    bwd_pass p = {h, params, images, in_dtype, preprocessing, n, height, width, dlogits, grads, ws, T, st};
    int rc = ubd_train_forward(p, logits);
    if (rc) return rc;
    rc = ubd_loss_impl(logits, h->k_out, y_true, (long)n * (height / 4) * (width / 4), loss, dlogits, ws + T.off_loss, st, h, h->cfg.dtype == UBD_BF16);
    if (rc) return rc;
    return ubd_train_backward(p);
}
