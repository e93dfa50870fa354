// Device pixel classification accuracy of the evaluation epoch on gfx950: class logits + label maps -> per-pixel correctness
// mask, pixel counts and the per-object accuracies of semantic_segmentation/evaluation.py:546-575
// (_calc_pixel_classification_correctness_mask), summed into a device accumulator.  No handle, no host synchronisation, no
// allocation; capturable in a HIP graph.
//
// Semantics reproduced (evaluation.py:546-575).  A call handles a batch of n maps of h x w, with labels t (int32, the y_true
// layout of ubd_loss) and class logits z[c], c = 0..C-1.
//   Mask and prediction
//     mask = t > 0.   true = t - 1 where mask, else 0.
//     pred = argmax_c z[c], with np.argmax's rule: the first maximum wins, and a NaN counts as the maximum, so the first NaN wins.
//     correct = (true == pred) at EVERY pixel, background included: a background pixel is "correct" iff pred == 0; a label
//     above C is simply never correct; a negative label is background.
//   Pixel counts
//     n_correct = sum of correct & mask.   n_total = sum of mask.
//   Objects
//     Objects are the external 8-connected components of mask, whatever class values they contain: two touching regions of
//     different classes are one object.  Every external component is an object, single pixels included (contourArea > -1
//     always holds).  An object's region is its FILLED contour: the component, plus every background pixel it encloses
//     (background is 4-connected), plus any components nested in those holes.  A nested component is NOT an object of its
//     own; its pixels count towards the enclosing object.  Object accuracy = sum of correct over the region / region size;
//     the hole pixels enter with the background rule above.
//   Correctness mask
//     +1 where mask & correct, -1 where mask & !correct, 0 elsewhere.
//   Dataset values
//     classification_pixel_acc_total = sum n_correct / sum n_total.  classification_pixel_acc_object = mean of the object
//     accuracies over all objects of all batches (the reference keeps a running weighted mean; here sums are kept and the
//     host divides once).
// The only cv2 parts of the routine are findContours(RETR_EXTERNAL) with min_area = -1 and drawContours(..., -1); both are
// restated as in postprocess.hip (external rule, filled contour = nesting chain), see its head and oracle/cv_post.c.
//
// Launches (ordered by the stream):
//   classify   grid over all pixels: argmax of the C strided class logits, correct, code byte (bit 0 mask, bit 1 correct) into
//              the workspace, optional int8 mask.  The logits are the call's dominant traffic (n h w stride 4 bytes against n h w 4
//              of labels): a wave fetches the contiguous float range of its 64 pixels with consecutive lanes on consecutive dwords
//              into an LDS stage and each lane scans its pixel's C values from there (pixel_stride <= 32; wider strides read
//              each lane's own contiguous C floats directly).
//   label      maps of at most 16384 pixels: ONE block per map, lock-free union-find forest in LDS (foreground 8-connected,
//              background 4-connected, frame node; the find / union of pp_lds.h), owner = raster-first pixel of the enclosing
//              external component, then integer (correct, size) counts per owner in LDS and the tail below -- one launch.
//              Larger maps: the same phases as launches of their own on a forest in global memory.
//   tail       per map, objects in raster order of their first pixel (the counters are indexed by that pixel, so a scan is the
//              order): correct / size in fp64, written to a compact list, summed by ONE wave left to right (as an unevaluated
//              pair of doubles, rounded once per map).
//   accumulate ONE block adds the per-image records, images in order, into the caller's accumulator: equal calls, equal bits.
// Integer atomics only (wave- or run-aggregated); no floating-point atomics, no grid-wide barrier.
#include "common.h"
#include "pp_lds.h"            // uf_find_wg / uf_union_wg: the project's lock-free union-find on an LDS forest

#define EP_MAX_CLASSES 31      // the evaluation's limit (UBD_MAX_CLASSES)
#define EP_THREADS 1024        // label / tail: one 16-wave block per map
#define EP_LDS_MAX_HW PP_LDS_MAX_HW
#define EP_CLS_THREADS 256
#define EP_STAGE_FLOATS 1024   // per wave: 64 pixels x stride <= 16, or 32 pixels x stride <= 32
#define EP_MAX_GRID 2048       // grid-stride kernels: at most 8 blocks per CU of a 256-CU device
#define EP_ACC_SLOTS 8         // 8-byte slots: n_correct, n_total, n_objects (int64), object_acc_sum (double), images (int64), 3 unused

// np.argmax over C floats: first maximum, first NaN wins
__device__ __forceinline__ int ep_argmax(const float *v, int C)
{
    float bv = v[0];
    int best = 0;
    for (int c = 1; c < C; ++c) {
        const float x = v[c];
        if ((x > bv || x != x) && bv == bv) { bv = x; best = c; }
    }
    return best;
}

// ------------------------------------------------------------------------------------ classify
// ppw: pixels a wave takes per round (64, or 32 when 64 x stride floats do not fit its stage); staged == 0: direct reads
__global__ __launch_bounds__(EP_CLS_THREADS) void ep_classify_kernel(const float *__restrict__ z, long stride, int C,
                                                                     const int32_t *__restrict__ labels, long npix, int ppw, int staged,
                                                                     unsigned char *__restrict__ code, int8_t *__restrict__ mask)
{
    __shared__ float stage[EP_CLS_THREADS / 64][EP_STAGE_FLOATS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float *st = stage[wid];
    const long rounds = (npix + ppw - 1) / ppw;
    const long nwaves = (long)gridDim.x * (EP_CLS_THREADS / 64);
    for (long r = (long)blockIdx.x * (EP_CLS_THREADS / 64) + wid; r < rounds; r += nwaves) {      // wave-uniform
        const long p0 = r * ppw;
        const int cnt = (int)(npix - p0 < ppw ? npix - p0 : ppw);
        const int t = lane < cnt ? labels[p0 + lane] : 0;
        int pred = 0;
        if (staged) {
            const int nfl = (cnt - 1) * (int)stride + C;            // the wave's pixels are one contiguous float range
            const float *src = z + p0 * stride;
            for (int i = lane; i < nfl; i += 64) st[i] = src[i];
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            if (lane < cnt) pred = ep_argmax(st + lane * (int)stride, C);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();                        // the next round overwrites the stage
        } else if (lane < cnt) {
            pred = ep_argmax(z + (p0 + lane) * stride, C);
        }
        if (lane < cnt) {
            const int m = t > 0 ? 1 : 0;
            const int truth = m ? t - 1 : 0;
            const int ok = truth == pred ? 1 : 0;
            code[p0 + lane] = (unsigned char)(m | (ok << 1));
            if (mask) mask[p0 + lane] = (int8_t)(m ? (ok ? 1 : -1) : 0);
        }
    }
}

// ------------------------------------------------------------------------------------ tail (shared by both forms)
// One block of NT threads, one map.  cnt[loc]: (correct << SHIFT) | size of the object whose raster-first pixel is loc, 0 where
// no object starts (an object's first pixel belongs to it: size >= 1).  wcnt: 2 * NT / 64 ints of LDS.  q: the map's list in
// global memory (root_cap doubles).  Writes the map's record; the list is summed left to right by wave 0.
template <int NT, typename CT, int SHIFT>
__device__ __forceinline__ void ep_image_tail(const CT *cnt, int hw, int *wcnt, double *q, long long n_correct, long long n_total,
                                              ubd_pixel_record *rec_ws, ubd_pixel_record *per_image)
{
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int base = 0, k = 0;
    for (int loc0 = 0; loc0 < hw; loc0 += NT, k ^= 1) {            // block-uniform; the two halves of wcnt alternate: one barrier per round
        const int loc = loc0 + tid;
        const CT c = loc < hw ? cnt[loc] : (CT)0;
        const bool obj = c != (CT)0;
        const unsigned long long b = __ballot(obj);
        if (lane == 0) wcnt[k * NW + wid] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int v = wcnt[k * NW + j];
            total += v;
            before += j < wid ? v : 0;
        }
        if (obj) {
            const long long size = (long long)(c & (((CT)1 << SHIFT) - 1)), corr = (long long)(c >> SHIFT);
            q[base + before + __popcll(b & ((1ull << lane) - 1ull))] = (double)corr / (double)size;
        }
        base += total;
    }
    __syncthreads();                                               // the list is complete (written and read by this block only)
    if (wid == 0) {
        // Fixed order: objects by raster position of their first pixel.  A plain fp64 running sum of hundreds of quotients rounds
        // at the size of the partial sum every time; the sum is kept as an unevaluated pair (Knuth's TwoSum: adds and subtracts
        // only, exact error term) and rounded once, so the record is within n_objects * 2^-52 of the exact rational sum:
        // <= 2^-54 per correctly rounded quotient (each <= 1) + one rounding of a sum <= n_objects.
        double s = 0.0, s_lo = 0.0;
        for (int b0 = 0; b0 < base; b0 += 64) {
            const double v = b0 + lane < base ? __hip_atomic_load(&q[b0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            const int cn = base - b0 < 64 ? base - b0 : 64;
            for (int j = 0; j < cn; ++j) {
                const double x = __shfl(v, j, 64);
                const double t = s + x, bb = t - s;
                s_lo += (s - (t - bb)) + (x - bb);
                s = t;
            }
        }
        if (lane == 0) {
            ubd_pixel_record r;
            r.n_correct = n_correct; r.n_total = n_total; r.n_objects = base; r.object_acc_sum = s + s_lo;
            *rec_ws = r;
            if (per_image) *per_image = r;
        }
    }
}

// ------------------------------------------------------------------------------------ label + count + tail, LDS form
// LDS (bytes): label int32 [hw + 1] | owner int16 [hw] + spare int16 [hw] (both: the union job queue of the merge phase) |
// code uint8 [hw] | n_correct, n_total, 2 unused, wave counts of the tail.  After the owner phase the label array is dead and
// holds the packed counters uint32 [hw] (size <= 16384 < 2^16).
static size_t ep_lds_bytes(int hw)
{
    return ubd_align_up(((size_t)hw + 1) * 4, 16) + (size_t)hw * 4 + ubd_align_up(hw, 16) + (4 + 2 * (EP_THREADS / 64)) * 4;
}

__global__ __launch_bounds__(EP_THREADS) void ep_label_lds_kernel(const unsigned char *__restrict__ code, int h, int w,
                                                                  double *__restrict__ objq, int root_cap,
                                                                  ubd_pixel_record *__restrict__ rec_ws, ubd_pixel_record *__restrict__ per_image)
{
    extern __shared__ __attribute__((aligned(16))) int smem[];
    constexpr int NT = EP_THREADS;
    const int img = blockIdx.x, hw = h * w, tid = threadIdx.x, lane = tid & 63;
    int *lab = smem;
    short *own16 = (short *)((char *)smem + ((((size_t)hw + 1) * 4 + 15) & ~(size_t)15));
    unsigned char *m = (unsigned char *)(own16 + 2 * (size_t)hw);
    int *ctr = (int *)(m + ((hw + 15) & ~15));
    const size_t pbase = (size_t)img * hw;
    // pixel -> row without an integer division: exact for loc < hw <= 2^14 (pp_lds.h)
    const float rcp_w = 1.0f / (float)w;
    auto row_of = [&](int loc) { return (int)(((float)loc + 0.5f) * rcp_w); };

    // ---- init: code bytes into LDS; a node per pixel (+ node 0 = frame / outside), pointed at the start of its horizontal run
    if (tid < 4) ctr[tid] = 0;
    for (int loc = tid; loc - lane < hw; loc += NT) {              // wave-uniform trip count
        const bool valid = loc < hw;
        int f = 0, x = 0;
        if (valid) {
            const int cd = code[pbase + loc];
            m[loc] = (unsigned char)cd;
            f = cd & 1;
            x = loc - row_of(loc) * w;
        }
        int fl = __shfl_up(f, 1, 64);
        if (lane == 0 && valid && x > 0) fl = code[pbase + loc - 1] & 1;
        const bool same_left = valid && x > 0 && fl == f;
        const unsigned long long breaks = __ballot(!same_left);
        if (valid) {
            const unsigned long long below = breaks & ((2ull << lane) - 1ull);
            const int start_off = below ? lane - (63 - __clzll(below)) : lane + 1;
            lab[loc + 1] = loc + 1 - start_off;
            if (loc == 0) lab[0] = 0;
        }
    }
    __syncthreads();

    // ---- merge: only the links the runs and a neighbour's links do not imply; foreground 8-connected, background 4-connected,
    // frame contact.  Queued as 16-bit jobs per wave and run 64 at a time where the queue fits (pp_lds.h, merge phase).
    {
        const int iters = (hw + NT - 1) / NT;
        const bool queued = (size_t)iters * NT <= (size_t)hw;
        unsigned short *queue = (unsigned short *)own16 + (size_t)(tid >> 6) * iters * 128;
        int njobs = 0;
        for (int loc = tid; loc - lane < hw; loc += NT) {
            int ja = -1, jb = -1;                                  // 0 N, 1 NW, 2 NE, 3 frame
            if (loc < hw) {
                const int y = row_of(loc), x = loc - y * w;
                const int c = m[loc] & 1;
                const bool W = x > 0 && (m[loc - 1] & 1) == c;
                if (c) {
                    if (y > 0) {
                        const bool N = m[loc - w] & 1;
                        const bool NW = x > 0 && (m[loc - w - 1] & 1);
                        if (N) {
                            if (!(W && NW)) ja = 0;
                        } else {
                            if (NW && !W) ja = 1;
                            const bool NE = x < w - 1 && (m[loc - w + 1] & 1);
                            const bool E = x < w - 1 && (m[loc + 1] & 1);
                            if (NE && !E) jb = 2;
                        }
                    }
                } else {
                    if (y > 0 && !(m[loc - w] & 1)) {
                        const bool NW = x > 0 && !(m[loc - w - 1] & 1);
                        if (!(W && NW)) ja = 0;
                    }
                    const bool row_edge = (y == 0 || y == h - 1) && !W;
                    if (row_edge || x == 0 || x == w - 1) jb = 3;
                }
            }
            if (queued) {
                const unsigned long long ba = __ballot(ja >= 0), bb = __ballot(jb >= 0);
                const unsigned long long below = (1ull << lane) - 1ull;
                if (ja >= 0) queue[njobs + __popcll(ba & below)] = (unsigned short)((loc << 2) | ja);
                njobs += __popcll(ba);
                if (jb >= 0) queue[njobs + __popcll(bb & below)] = (unsigned short)((loc << 2) | jb);
                njobs += __popcll(bb);
            } else {
                const int me = loc + 1;
                if (ja >= 0) uf_union_wg(lab, me, ja == 0 ? me - w : me - w - 1);
                if (jb >= 0) uf_union_wg(lab, me, jb == 2 ? me - w + 1 : 0);
            }
        }
        if (queued) {
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            for (int j = lane; j < njobs; j += 64) {
                const int job = queue[j], me = (job >> 2) + 1, dir = job & 3;
                uf_union_wg(lab, me, dir == 0 ? me - w : (dir == 1 ? me - w - 1 : (dir == 2 ? me - w + 1 : 0)));
            }
        }
    }
    __syncthreads();

    // ---- flatten with a READ-ONLY find: the only stores are true roots into the thread's own nodes (pp_lds.h, flatten phase)
    for (int node0 = tid; node0 <= hw; node0 += 4 * NT) {
        int cur[4];
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { cur[k] = node0 + k * NT; live[k] = cur[k] <= hw; if (!live[k]) cur[k] = 0; }
        for (;;) {
            int nxt[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) nxt[k] = __hip_atomic_load(&lab[cur[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            bool moved = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) { moved |= nxt[k] != cur[k]; cur[k] = nxt[k]; }
            if (!moved) break;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (live[k]) __hip_atomic_store(&lab[node0 + k * NT], cur[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();

    // ---- owner: the raster-first pixel of the enclosing external component, or -1.  A region's raster-first pixel (its root)
    // walks the nesting chain -- region -> region north of its first pixel -> ... ; every step moves to a smaller node -- and the
    // other pixels copy their root's entry after a barrier: they write entries nobody reads, so the copy is in place.
    for (int loc = tid; loc < hw; loc += NT) {
        if (lab[loc + 1] != loc + 1) continue;
        int node = loc + 1, own = -1;
        for (;;) {
            if (node == 0) break;                                   // outside background
            const int r = node - 1;
            if (r < w) { if (m[r] & 1) own = r; break; }
            const int up = lab[r - w + 1];
            if ((m[r] & 1) && up == 0) { own = r; break; }          // external: north of its first pixel is outside background
            node = up;
        }
        own16[loc] = (short)own;
    }
    __syncthreads();
    for (int loc = tid; loc < hw; loc += NT) {
        const int node = lab[loc + 1];
        if (node == loc + 1) continue;
        own16[loc] = node == 0 ? (short)-1 : own16[node - 1];
    }
    __syncthreads();
    unsigned *cnt = (unsigned *)lab;                               // the forest is dead from here on
    for (int loc = tid; loc < hw; loc += NT) cnt[loc] = 0u;
    __syncthreads();

    // ---- count: (correct << 16) + 1 per pixel of a region, into the counter at the owner's pixel.  A thread's pixels lie NT / w
    // rows apart, usually inside one object: summed in a register while the owner does not change, one LDS atomic per run.
    {
        int run_key = -1, n_ok = 0, n_fg = 0;
        unsigned run_sum = 0u;
        for (int loc = tid; loc < hw; loc += NT) {
            const int cd = m[loc];
            n_fg += cd & 1;
            n_ok += cd == 3 ? 1 : 0;
            const int o = own16[loc];
            if (o < 0) continue;
            if (o != run_key) {
                if (run_sum != 0u) atomicAdd(&cnt[run_key], run_sum);
                run_key = o; run_sum = 0u;
            }
            run_sum += 1u + ((unsigned)(cd >> 1) << 16);
        }
        if (run_sum != 0u) atomicAdd(&cnt[run_key], run_sum);
        for (int o = 32; o > 0; o >>= 1) { n_ok += __shfl_xor(n_ok, o, 64); n_fg += __shfl_xor(n_fg, o, 64); }
        if (lane == 0) { atomicAdd(&ctr[0], n_ok); atomicAdd(&ctr[1], n_fg); }
    }
    __syncthreads();
    ep_image_tail<NT, unsigned, 16>(cnt, hw, ctr + 4, objq + (size_t)img * root_cap, (long long)ctr[0], (long long)ctr[1],
                                    rec_ws + img, per_image ? per_image + img : nullptr);
}

// ------------------------------------------------------------------------------------ global-memory form (maps above 16384 pixels)
// The phases of the LDS form as launches over all pixels of the chunk (n * hw < 2^31), forest in global memory.
__device__ __forceinline__ int ep_uf_find(int *lab, int a)
{
    int p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != a) {
        a = p;
        p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return a;
}

__device__ __forceinline__ void ep_uf_union(int *lab, int a, int b)
{
    for (;;) {
        a = ep_uf_find(lab, a);
        b = ep_uf_find(lab, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }          // a > b: hang a under b
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;                                         // a was no longer a root: retry with its parent
    }
}

// blockDim a multiple of 64; the lanes of a wave hold 64 consecutive flat pixels
// also clears the counters (a kernel's stores, not a memset node, when the call is captured in a graph)
__global__ __launch_bounds__(256) void ep_init_kernel(const unsigned char *__restrict__ code, long npix, int hw, int w, int *__restrict__ label,
                                                      unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const long nround = (npix + 63) / 64 * 64;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nround; p += (long)gridDim.x * blockDim.x) {
        const bool valid = p < npix;
        int f = 0, img = 0, loc = 0, x = 0;
        if (valid) {
            img = (int)(p / hw); loc = (int)(p % hw); x = loc % w;
            f = code[p] & 1;
            cnt[p] = 0ull;
        }
        int fl = __shfl_up(f, 1, 64);
        if (lane == 0 && valid && x > 0) fl = code[p - 1] & 1;
        const bool same_left = valid && x > 0 && fl == f;
        const unsigned long long breaks = __ballot(!same_left);  // bit l: lane l starts a run (or is invalid)
        if (valid) {
            const unsigned long long below = breaks & ((2ull << lane) - 1ull);
            const int start_off = below ? lane - (63 - __clzll(below)) : lane + 1;   // or the run continues into the previous wave: link there
            int *lab = label + (size_t)img * (hw + 1);
            lab[loc + 1] = loc + 1 - start_off;
            if (loc == 0) lab[0] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void ep_merge_kernel(const unsigned char *__restrict__ code, int *__restrict__ label, long npix, int h, int w)
{
    const int hw = h * w;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const int img = (int)(p / hw), loc = (int)(p % hw);
        const int y = loc / w, x = loc % w;
        const unsigned char *m = code + (size_t)img * hw;
        int *lab = label + (size_t)img * (hw + 1);
        const int me = loc + 1;
        const int c = m[loc] & 1;
        const bool W = x > 0 && (m[loc - 1] & 1) == c;
        if (c) {
            if (y > 0) {
                const bool N = m[loc - w] & 1;
                const bool NW = x > 0 && (m[loc - w - 1] & 1);
                if (N) {
                    if (!(W && NW)) ep_uf_union(lab, me, me - w);
                } else {
                    if (NW && !W) ep_uf_union(lab, me, me - w - 1);
                    const bool NE = x < w - 1 && (m[loc - w + 1] & 1);
                    const bool E = x < w - 1 && (m[loc + 1] & 1);
                    if (NE && !E) ep_uf_union(lab, me, me - w + 1);
                }
            }
        } else {
            if (y > 0 && !(m[loc - w] & 1)) {
                const bool NW = x > 0 && !(m[loc - w - 1] & 1);
                if (!(W && NW)) ep_uf_union(lab, me, me - w);
            }
            // frame contact: one link per run on the first / last row, the row ends elsewhere
            const bool row_edge = (y == 0 || y == h - 1) && !W;
            if (row_edge || x == 0 || x == w - 1) ep_uf_union(lab, me, 0);
        }
    }
}

__global__ __launch_bounds__(256) void ep_flatten_kernel(int *__restrict__ label, int n, int hw)
{
    const long total = (long)n * (hw + 1);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int img = (int)(p / (hw + 1)), node = (int)(p % (hw + 1));
        int *lab = label + (size_t)img * (hw + 1);
        const int r = ep_uf_find(lab, node);              // read-only find: the only store is the node's own root
        __hip_atomic_store(&lab[node], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// owner pixel per pixel + the counts: (correct << 32) + 1 into the counter at the owner's pixel, one atomic per distinct
// owner in the wave
__global__ __launch_bounds__(256) void ep_owner_count_kernel(const unsigned char *__restrict__ code, const int *__restrict__ label,
                                                             long npix, int h, int w, unsigned long long *__restrict__ cnt)
{
    const int hw = h * w, lane = threadIdx.x & 63;
    const long nround = (npix + 63) / 64 * 64;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nround; p += (long)gridDim.x * blockDim.x) {
        int key = -1;
        unsigned long long val = 0ull;
        if (p < npix) {
            const int img = (int)(p / hw), loc = (int)(p % hw);
            const unsigned char *m = code + (size_t)img * hw;
            const int *lab = label + (size_t)img * (hw + 1);
            int node = lab[loc + 1], own = -1;
            for (;;) {                                      // the forest is flat; every step moves to a smaller node
                if (node == 0) break;                       // outside background
                const int r = node - 1;                     // raster-first pixel of this region
                if (r < w) { if (m[r] & 1) own = r; break; }
                const int up = lab[r - w + 1];              // region north of it
                if ((m[r] & 1) && up == 0) { own = r; break; }
                node = up;
            }
            if (own >= 0) {
                key = img * hw + own;                       // < 2^31 (chunked by the host)
                val = 1ull + ((unsigned long long)(m[loc] >> 1) << 32);
            }
        }
        unsigned long long todo = __ballot(key >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k = __shfl(key, leader, 64);
            const bool mine = key == k;
            unsigned long long v = mine ? val : 0ull;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == leader) atomicAdd(&cnt[k], v);
            todo &= ~__ballot(mine);
        }
    }
}

__global__ __launch_bounds__(EP_THREADS) void ep_image_tail_kernel(const unsigned char *__restrict__ code, const unsigned long long *cnt,
                                                                   int hw, double *__restrict__ objq, int root_cap,
                                                                   ubd_pixel_record *__restrict__ rec_ws, ubd_pixel_record *__restrict__ per_image)
{
    __shared__ int s[4 + 2 * (EP_THREADS / 64)];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (tid < 4) s[tid] = 0;
    __syncthreads();
    int n_ok = 0, n_fg = 0;
    for (int loc = tid; loc < hw; loc += EP_THREADS) {
        const int cd = code[(size_t)img * hw + loc];
        n_fg += cd & 1;
        n_ok += cd == 3 ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) { n_ok += __shfl_xor(n_ok, o, 64); n_fg += __shfl_xor(n_fg, o, 64); }
    if (lane == 0) { atomicAdd(&s[0], n_ok); atomicAdd(&s[1], n_fg); }
    __syncthreads();
    ep_image_tail<EP_THREADS, unsigned long long, 32>(cnt + (size_t)img * hw, hw, s + 4, objq + (size_t)img * root_cap, (long long)s[0],
                                                      (long long)s[1], rec_ws + img, per_image ? per_image + img : nullptr);
}

// ------------------------------------------------------------------------------------ accumulate
// ONE wave: integer sums in any order, the fp64 sum image by image behind what the accumulator already holds
__global__ __launch_bounds__(64) void ep_accumulate_kernel(const ubd_pixel_record *__restrict__ rec, int m, void *accumulator)
{
    int64_t *ai = (int64_t *)accumulator;
    double *ad = (double *)accumulator;
    const int lane = threadIdx.x;
    long long n_ok = 0, n_fg = 0, n_obj = 0;
    double s = ad[3];
    for (int b0 = 0; b0 < m; b0 += 64) {
        ubd_pixel_record r;
        r.n_correct = 0; r.n_total = 0; r.n_objects = 0; r.object_acc_sum = 0.0;
        if (b0 + lane < m) r = rec[b0 + lane];
        n_ok += r.n_correct; n_fg += r.n_total; n_obj += r.n_objects;
        const int cn = m - b0 < 64 ? m - b0 : 64;
        for (int j = 0; j < cn; ++j) s += __shfl(r.object_acc_sum, j, 64);
    }
    for (int o = 32; o > 0; o >>= 1) { n_ok += __shfl_xor(n_ok, o, 64); n_fg += __shfl_xor(n_fg, o, 64); n_obj += __shfl_xor(n_obj, o, 64); }
    if (lane == 0) { ai[0] += n_ok; ai[1] += n_fg; ai[2] += n_obj; ad[3] = s; ai[4] += m; }
}

// ------------------------------------------------------------------------------------ host
struct ep_layout {
    size_t off_rec;        // ubd_pixel_record [m]
    size_t off_code;       // uint8 [m][hw]: bit 0 mask, bit 1 correct
    size_t off_q;          // double [m][root_cap]: object accuracies of a map in raster order
    size_t off_cnt;        // global form: uint64 [m][hw] (cleared by the init launch)
    size_t off_label;      // global form: int32 [m][hw + 1]
    size_t total;
    int root_cap, chunk;   // chunk: images per pass (chunk * hw < 2^31)
};

static bool ep_sizes_ok(int n, int h, int w) { return n >= 1 && h >= 1 && w >= 1 && h < 32768 && w < 32768; }

static void ep_layout_compute(int n, int h, int w, ep_layout *L)
{
    const size_t hw = (size_t)h * w;
    const long per = (long)(((1L << 31) - 1) / (long)hw);
    const size_t m = (size_t)((long)n < per ? (long)n : per);
    size_t off = 0;
    L->chunk = (int)m;
    L->root_cap = ((h + 1) / 2) * ((w + 1) / 2) + 1;              // most external components a map can hold (+ 1)
    L->off_rec = off;   off += ubd_align_up(sizeof(ubd_pixel_record) * m, 256);
    L->off_code = off;  off += ubd_align_up(m * hw, 256);
    L->off_q = off;     off += ubd_align_up(sizeof(double) * m * (size_t)L->root_cap, 256);
    L->off_cnt = off;
    L->off_label = off;
    if (hw > EP_LDS_MAX_HW) {
        off += ubd_align_up(sizeof(unsigned long long) * m * hw, 256);
        L->off_label = off; off += ubd_align_up(sizeof(int) * m * (hw + 1), 256);
    }
    L->total = off;
}

extern "C" size_t ubd_evaluate_pixels_accumulator_bytes(void) { return (size_t)EP_ACC_SLOTS * 8; }

extern "C" size_t ubd_evaluate_pixels_workspace_bytes(int n, int map_h, int map_w)
{
    if (!ep_sizes_ok(n, map_h, map_w)) return 0;
    ep_layout L;
    ep_layout_compute(n, map_h, map_w, &L);
    return L.total;
}

extern "C" int ubd_evaluate_pixels(const float *class_logits, int pixel_stride, int n_classes, const int32_t *labels, int n, int map_h,
                                   int map_w, int8_t *mask, ubd_pixel_record *per_image, void *accumulator, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    UBD_REQUIRE(class_logits && labels, "ubd_evaluate_pixels: null argument");
    UBD_REQUIRE(accumulator, "ubd_evaluate_pixels: null accumulator");
    UBD_REQUIRE(workspace, "ubd_evaluate_pixels: null workspace");
    UBD_REQUIRE(n_classes >= 1 && n_classes <= EP_MAX_CLASSES, "ubd_evaluate_pixels: n_classes must be 1..%d, got %d", EP_MAX_CLASSES, n_classes);
    UBD_REQUIRE(pixel_stride >= n_classes, "ubd_evaluate_pixels: pixel_stride %d is below n_classes %d", pixel_stride, n_classes);
    UBD_REQUIRE(n >= 1, "ubd_evaluate_pixels: n must be >= 1, got %d", n);
    UBD_REQUIRE(map_h >= 1 && map_w >= 1, "ubd_evaluate_pixels: bad sizes h=%d w=%d", map_h, map_w);
    UBD_REQUIRE(map_h < 32768 && map_w < 32768, "ubd_evaluate_pixels: map too large");
    ep_layout L;
    ep_layout_compute(n, map_h, map_w, &L);
    UBD_REQUIRE(workspace_bytes >= L.total, "ubd_evaluate_pixels: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int hw = map_h * map_w;
    const bool lds_form = hw <= EP_LDS_MAX_HW;
    if (lds_form) {                                              // the kernel's dynamic-LDS limit, once per device
        static bool attr_set[64];
        int dev = 0;
        UBD_CHECK_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !attr_set[dev]) {
            UBD_CHECK_HIP(hipFuncSetAttribute((const void *)ep_label_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ep_lds_bytes(EP_LDS_MAX_HW)));
            if (dev >= 0 && dev < 64) attr_set[dev] = true;
        }
    }
    ubd_pixel_record *rec = (ubd_pixel_record *)(ws + L.off_rec);
    unsigned char *code = (unsigned char *)(ws + L.off_code);
    double *objq = (double *)(ws + L.off_q);
    const int staged = pixel_stride <= 32;
    const int ppw = !staged || pixel_stride <= EP_STAGE_FLOATS / 64 ? 64 : 32;
    for (int i0 = 0; i0 < n; i0 += L.chunk) {
        const int m = n - i0 < L.chunk ? n - i0 : L.chunk;
        const long npix = (long)m * hw;
        const size_t p0 = (size_t)i0 * hw;
        ubd_pixel_record *pi = per_image ? per_image + i0 : nullptr;
        const long rounds = (npix + ppw - 1) / ppw;
        long cgrid = (rounds + EP_CLS_THREADS / 64 - 1) / (EP_CLS_THREADS / 64);
        if (cgrid > EP_MAX_GRID) cgrid = EP_MAX_GRID;
        hipLaunchKernelGGL(ep_classify_kernel, dim3((unsigned)cgrid), dim3(EP_CLS_THREADS), 0, st, class_logits + p0 * (size_t)pixel_stride,
                           (long)pixel_stride, n_classes, labels + p0, npix, ppw, staged, code, mask ? mask + p0 : nullptr);
        if (lds_form) {
            hipLaunchKernelGGL(ep_label_lds_kernel, dim3(m), dim3(EP_THREADS), ep_lds_bytes(hw), st, (const unsigned char *)code, map_h, map_w,
                               objq, L.root_cap, rec, pi);
        } else {
            unsigned long long *cnt = (unsigned long long *)(ws + L.off_cnt);
            int *label = (int *)(ws + L.off_label);
            long grid = (npix + 255) / 256;
            if (grid > EP_MAX_GRID) grid = EP_MAX_GRID;
            hipLaunchKernelGGL(ep_init_kernel, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned char *)code, npix, hw, map_w, label, cnt);
            hipLaunchKernelGGL(ep_merge_kernel, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned char *)code, label, npix, map_h, map_w);
            hipLaunchKernelGGL(ep_flatten_kernel, dim3((unsigned)grid), dim3(256), 0, st, label, m, hw);
            hipLaunchKernelGGL(ep_owner_count_kernel, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned char *)code, (const int *)label, npix,
                               map_h, map_w, cnt);
            hipLaunchKernelGGL(ep_image_tail_kernel, dim3(m), dim3(EP_THREADS), 0, st, (const unsigned char *)code,
                               (const unsigned long long *)cnt, hw, objq, L.root_cap, rec, pi);
        }
        hipLaunchKernelGGL(ep_accumulate_kernel, dim3(1), dim3(64), 0, st, (const ubd_pixel_record *)rec, m, accumulator);
        UBD_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
