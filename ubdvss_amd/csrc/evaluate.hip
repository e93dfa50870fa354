// Object-level evaluation on the device (ubd_evaluate_objects): found quads + ground-truth polygons -> IoU tables -> the
// 1-1 / 1-many / many-1 matching of FtMetricsCalculator.analyze (evaluation.py:229-328) -> per-threshold counters, summed into a
// caller-owned accumulator.  All geometry in fp64, without FMA contraction (build.sh), so exact inputs give exact cross products.
//
// One geometric primitive serves every area: ev_edge_interval clips the segment a->b to a convex counter-clockwise polygon and
// returns the covered parameter interval [lo, hi] of the segment.  With it
//   area(A and B)     = sum over the edges of A of their part inside B + sum over the edges of B of their part inside A,
//   area(P1 or .. Pm) = sum over the edges of every Pi of the part covered by no other Pj,
// each part weighted with cross(a - r, b - r) / 2 (Green's theorem; r is a reference vertex near the polygons so that the
// products stay of the size of the polygons, not of the image).  Areas of a union intersected with a box or with another
// union follow by inclusion-exclusion from three union areas.
// Tie rule for collinear edges (the normal case with integer quads): two edges of the SAME direction share their common part,
// which only the polygon with the lower index keeps (union) / counts (intersection); two edges of OPPOSITE direction lie on
// opposite sides of the line: both keep the part in a union (the two contributions cancel), neither counts it in an intersection.
// Polygon index = slot in the image's polygon list: ground truths first, found quads after them.  Zero-area polygons cover
// nothing and contribute nothing.
//
// Launches per call (and per 64 images): prepare (rescale, winding, areas) -> tables (one wave per ground-truth row, lanes over
// found quads) -> match (one block per image: adjacency, classes of correspondences, group and by-area unions, records) ->
// accumulate (ONE block walks the images in order: bit-identical sums run to run; no floating-point atomics).
//
// Two entries share the kernels through template <int MAXV>, the vertices a polygon slot of the workspace holds: ubd_evaluate_objects
// (MAXV = UBD_EVAL_MAX_VERTS = 8, ground truth of 3..8 vertices) and ubd_evaluate_polygons (MAXV = UBD_POLY_MAX_VERTS = 64, hulls
// read from segmentation maps).  Only the slot stride and the prepare phase's staging differ: at 8 vertices a polygon is
// normalised in registers, at 64 in its workspace slot (1 KB per thread would go to scratch).  The work units of a union are
// (polygon, edge) numbered polygon * MAXV + edge and dealt to the EV_WAVES waves round robin: MAXV is a multiple of EV_WAVES, so
// an edge lands in the same wave, in the same order, for either MAXV, and the two entries give the same bits on common ground.
#include "common.h"
#include <algorithm>

#define EV_MAX_GT UBD_EVAL_MAX_GT
#define EV_MAX_FOUND UBD_EVAL_MAX_FOUND
#define EV_MAX_V UBD_EVAL_MAX_VERTS
#define EV_MAX_T UBD_EVAL_MAX_THRESHOLDS
#define EV_MAX_IMGS 64
#define EV_THREADS 256
#define EV_WAVES (EV_THREADS / 64)
#define EV_ADJ_IOU 0.05                       // iou_precision_threshold, evaluation.py:235
#define EV_ACC_HEAD 8                         // accumulator: 8 slots of 8 bytes, then 10 per threshold, then the confusion sums
#define EV_ACC_PER_T 10

struct ev_layout {                            // workspace carving, offsets in bytes
    int P;                                    // polygon slots per image = max_gt + cap
    size_t off_xy;                            // double (n, P, 2 * MAXV)
    size_t off_nv;                            // int32  (n, P)   vertex count, 0 = not a polygon of this image
    size_t off_tab;                           // double (n, tab_stride): areas gt [max_gt], areas found [cap], inter [max_gt][cap], iou [max_gt][cap]
    size_t tab_stride;                        // doubles per image
    size_t off_rec;                           // ubd_eval_record (n, T)
    size_t off_cm;                            // double (n, T, C, C)
    size_t total;
};

static void ev_layout_compute(int n, int max_gt, int cap, int T, int C, int maxv, ev_layout *L)
{
    L->P = max_gt + cap;
    size_t o = 0;
    L->off_xy = o; o = ubd_align_up(o + (size_t)n * L->P * 2 * maxv * sizeof(double), 256);
    L->off_nv = o; o = ubd_align_up(o + (size_t)n * L->P * sizeof(int32_t), 256);
    L->tab_stride = (size_t)max_gt + cap + 2 * (size_t)max_gt * cap;
    L->off_tab = o; o = ubd_align_up(o + (size_t)n * L->tab_stride * sizeof(double), 256);
    L->off_rec = o; o = ubd_align_up(o + (size_t)n * T * sizeof(ubd_eval_record), 256);
    L->off_cm = o; o = ubd_align_up(o + (size_t)n * T * C * C * sizeof(double), 256);
    L->total = o;
}

struct ev_launch {                            // by value: the HOST arrays of the call travel in the kernel arguments
    int m;                                    // images of this launch
    int img0;                                 // first image of this launch within the call
    int max_gt, cap, T, C;
    int max_verts;                            // most vertices a ground-truth polygon may have (<= MAXV)
    int n_gt_verts;                           // vertices in gt_xy: every polygon's vertex range [gt_first[p], gt_first[p + 1]) is checked against it
                                              // (gt_first itself is the caller's: total_gt + 1 entries, indexed by the HOST image_first values only)
    int gt0[EV_MAX_IMGS + 1];                 // first ground-truth polygon of each image
    double thr[EV_MAX_T];
};

struct ev_image {                             // one image's views
    const double *xy;                         // (P, 2 * MAXV)
    const int32_t *nv;                        // (P)
    const double *area_g, *area_f;            // [max_gt], [cap]
    const double *inter, *iou;                // [max_gt][cap]
    int G, F, cap, max_gt;
};

// Part of the segment a -> b inside the convex counter-clockwise polygon P (nv vertices, x0,y0,x1,y1,...): true and [lo, hi]
// with lo < hi, or false.  same_inside: a polygon edge collinear with the segment and of the same direction does not bound it.
__device__ __forceinline__ bool ev_edge_interval(double ax, double ay, double bx, double by, const double *__restrict__ P, int nv,
                                                 bool same_inside, double &lo, double &hi)
{
    lo = 0.0; hi = 1.0;
    double px = P[2 * (nv - 1)], py = P[2 * (nv - 1) + 1];
    for (int k = 0; k < nv; ++k) {
        const double qx = P[2 * k], qy = P[2 * k + 1];
        const double ex = qx - px, ey = qy - py;
        const double d0 = ex * (ay - py) - ey * (ax - px);
        const double d1 = ex * (by - py) - ey * (bx - px);
        px = qx; py = qy;
        if (ex == 0.0 && ey == 0.0) continue;                              // repeated vertex
        if (d0 == 0.0 && d1 == 0.0) {
            if (same_inside && ex * (bx - ax) + ey * (by - ay) > 0.0) continue;
            return false;
        }
        if (d0 <= 0.0 && d1 <= 0.0) return false;                          // outside, or touching in one point
        if (d0 < 0.0) lo = fmax(lo, d0 / (d0 - d1));
        else if (d1 < 0.0) hi = fmin(hi, d0 / (d0 - d1));
    }
    return lo < hi;
}

__device__ __forceinline__ double ev_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

__device__ __forceinline__ double ev_iou(double a1, double a2, double inter)      // evaluation.py:424-429
{
    const double u = a1 + a2 - inter;
    return u > 0.0 ? inter / u : 0.0;
}

// shoelace with the first vertex as origin: the same sum the intersection of a polygon with itself produces
__device__ __forceinline__ double ev_signed_area(const double *P, int nv)
{
    double s = 0.0;
    const double rx = P[0], ry = P[1];
    for (int k = 0; k < nv; ++k) {
        const int k1 = k + 1 == nv ? 0 : k + 1;
        s += 0.5 * ev_cross(P[2 * k] - rx, P[2 * k + 1] - ry, P[2 * k1] - rx, P[2 * k1 + 1] - ry);
    }
    return s;
}

// ---- phase 1: polygons of the call -> counter-clockwise fp64 polygons + areas; record flags ------------------------------------
template <int MAXV>
__global__ __launch_bounds__(EV_THREADS) void ev_prepare_kernel(const int32_t *__restrict__ quads, const int32_t *__restrict__ counts,
                                                                const double *__restrict__ scales, const double *__restrict__ gt_xy,
                                                                const int32_t *__restrict__ gt_first, char *__restrict__ ws,
                                                                ev_layout L, ev_launch A, int32_t *__restrict__ flags)
{
    const int li = blockIdx.x, img = A.img0 + li;
    const int G = A.gt0[li + 1] - A.gt0[li];
    const int cnt = counts[img];
    const bool overflow = cnt > A.cap || cnt < 0;
    const int F = overflow ? 0 : cnt;
    double *xy = (double *)(ws + L.off_xy) + (size_t)img * L.P * (2 * MAXV);
    int32_t *nvv = (int32_t *)(ws + L.off_nv) + (size_t)img * L.P;
    double *tab = (double *)(ws + L.off_tab) + (size_t)img * L.tab_stride;
    constexpr bool IN_REGS = MAXV <= EV_MAX_V;          // else the polygon is normalised in its workspace slot
    __shared__ int bad;
    if (threadIdx.x == 0) bad = overflow ? 1 : 0;
    __syncthreads();
    for (int s = threadIdx.x; s < L.P; s += EV_THREADS) {
        double regs[IN_REGS ? 2 * MAXV : 2];
        double *v = IN_REGS ? regs : xy + (size_t)s * (2 * MAXV);
        int nv = 0;
        if (s < A.max_gt) {
            if (s < G) {
                const int p = A.gt0[li] + s;
                const int v0 = gt_first[p], v1 = gt_first[p + 1];
                nv = v1 - v0;
                if (v0 < 0 || nv < 3 || nv > A.max_verts || v1 > A.n_gt_verts) { nv = 0; atomicOr(&bad, 2); }
                for (int k = 0; k < nv; ++k) { v[2 * k] = gt_xy[2 * (size_t)(v0 + k)]; v[2 * k + 1] = gt_xy[2 * (size_t)(v0 + k) + 1]; }
            }
        } else if (s - A.max_gt < F) {
            const int32_t *q = quads + ((size_t)img * A.cap + (s - A.max_gt)) * 8;
            nv = 4;
            for (int k = 0; k < 4; ++k) {
                double x = (double)q[2 * k], y = (double)q[2 * k + 1];
                if (scales) {                                   // utils.py:67-69: int(coordinate * scale), truncation toward zero
                    x = trunc(x * scales[2 * img]);
                    y = trunc(y * scales[2 * img + 1]);
                }
                v[2 * k] = x; v[2 * k + 1] = y;
            }
        }
        double area = 0.0;
        if (nv) {
            area = ev_signed_area(v, nv);
            if (area < 0.0) {                                   // clockwise -> counter-clockwise, first vertex kept
                for (int k = 1; k < nv - k; ++k) {
                    const double tx = v[2 * k], ty = v[2 * k + 1];
                    v[2 * k] = v[2 * (nv - k)]; v[2 * k + 1] = v[2 * (nv - k) + 1];
                    v[2 * (nv - k)] = tx; v[2 * (nv - k) + 1] = ty;
                }
                area = ev_signed_area(v, nv);
            }
        }
        if (IN_REGS)
            for (int k = 0; k < nv; ++k) { xy[(size_t)s * (2 * MAXV) + 2 * k] = v[2 * k]; xy[(size_t)s * (2 * MAXV) + 2 * k + 1] = v[2 * k + 1]; }
        nvv[s] = nv;
        if (s < A.max_gt) tab[s] = area; else tab[A.max_gt + (s - A.max_gt)] = area;
    }
    __syncthreads();
    if (threadIdx.x == 0) flags[img] = bad;
}

// ---- phase 2: G x F intersection and IoU tables (evaluation.py:210-227); one wave per ground-truth row ---------------------------
template <int MAXV>
__global__ __launch_bounds__(64) void ev_tables_kernel(const int32_t *__restrict__ counts, char *__restrict__ ws, ev_layout L, ev_launch A)
{
    const int li = blockIdx.y, img = A.img0 + li, g = blockIdx.x;
    const int G = A.gt0[li + 1] - A.gt0[li];
    if (g >= G) return;
    const int cnt = counts[img];
    const int F = (cnt > A.cap || cnt < 0) ? 0 : cnt;
    const double *xy = (const double *)(ws + L.off_xy) + (size_t)img * L.P * (2 * MAXV);
    const int32_t *nvv = (const int32_t *)(ws + L.off_nv) + (size_t)img * L.P;
    double *tab = (double *)(ws + L.off_tab) + (size_t)img * L.tab_stride;
    double *inter_t = tab + A.max_gt + A.cap, *iou_t = inter_t + (size_t)A.max_gt * A.cap;
    const double *Pg = xy + (size_t)g * (2 * MAXV);
    const int ng = nvv[g];
    const double ag = tab[g];
    for (int f = threadIdx.x; f < F; f += 64) {
        const double *Pf = xy + (size_t)(A.max_gt + f) * (2 * MAXV);
        const int nf = nvv[A.max_gt + f];
        const double af = tab[A.max_gt + f];
        double inter = 0.0;
        if (ng && nf && ag > 0.0 && af > 0.0) {
            const double rx = Pg[0], ry = Pg[1];
            double lo, hi;
            for (int k = 0; k < ng; ++k) {                      // edges of the ground truth (the lower index) inside the found quad
                const int k1 = k + 1 == ng ? 0 : k + 1;
                const double ax = Pg[2 * k], ay = Pg[2 * k + 1], bx = Pg[2 * k1], by = Pg[2 * k1 + 1];
                if (ev_edge_interval(ax, ay, bx, by, Pf, nf, true, lo, hi))
                    inter += (hi - lo) * (0.5 * ev_cross(ax - rx, ay - ry, bx - rx, by - ry));
            }
            for (int k = 0; k < nf; ++k) {
                const int k1 = k + 1 == nf ? 0 : k + 1;
                const double ax = Pf[2 * k], ay = Pf[2 * k + 1], bx = Pf[2 * k1], by = Pf[2 * k1 + 1];
                if (ev_edge_interval(ax, ay, bx, by, Pg, ng, false, lo, hi))
                    inter += (hi - lo) * (0.5 * ev_cross(ax - rx, ay - ry, bx - rx, by - ry));
            }
            inter = fmin(fmax(inter, 0.0), fmin(ag, af));
        }
        inter_t[(size_t)g * A.cap + f] = inter;
        iou_t[(size_t)g * A.cap + f] = ev_iou(ag, af, inter);
    }
}

// ---- area of a union of convex polygons, by the whole block ----------------------------------------------------------------------
// list[0..m): polygon slots.  ivl: this wave's LDS interval list (2 * (EV_MAX_GT + EV_MAX_FOUND) doubles).  Every thread returns
// the same value.  Work unit = (polygon, edge): waves take units round robin, lanes walk the other polygons; the fixed assignment
// and the fixed reduction trees make the sum independent of timing.
template <int MAXV>
__device__ double ev_union_area(const ev_image &im, const short *list, int m, double *ivl, double *wsum)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc = 0.0;
    if (m > 0) {
        const double *P0 = im.xy + (size_t)list[0] * (2 * MAXV);
        const double rx = P0[0], ry = P0[1];
        for (int u = w; u < m * MAXV; u += EV_WAVES) {
            const int is = u / MAXV, e = u % MAXV;
            const int si = list[is];
            const int nvi = im.nv[si];
            const double ai = si < im.max_gt ? im.area_g[si] : im.area_f[si - im.max_gt];
            if (e >= nvi || !(ai > 0.0)) continue;
            const double *Pi = im.xy + (size_t)si * (2 * MAXV);
            const int e1 = e + 1 == nvi ? 0 : e + 1;
            const double ax = Pi[2 * e], ay = Pi[2 * e + 1], bx = Pi[2 * e1], by = Pi[2 * e1 + 1];
            if (ax == bx && ay == by) continue;
            int K = 0;
            for (int jb = 0; jb < m; jb += 64) {
                const int js = jb + lane;
                bool have = false;
                double lo = 0.0, hi = 0.0;
                if (js < m && js != is) {
                    const int sj = list[js];
                    const double aj = sj < im.max_gt ? im.area_g[sj] : im.area_f[sj - im.max_gt];
                    if (aj > 0.0) have = ev_edge_interval(ax, ay, bx, by, im.xy + (size_t)sj * (2 * MAXV), im.nv[sj], sj < si, lo, hi);
                }
                const unsigned long long mask = __ballot(have);
                if (have) {
                    const int pos = K + __popcll(mask & ((1ull << lane) - 1ull));
                    ivl[2 * pos] = lo; ivl[2 * pos + 1] = hi;
                }
                K += __popcll(mask);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // uncovered measure of [0, 1]: a gap starts at 0 or at the end of an interval, where no interval covers the point,
            // and runs to the next interval start (or 1); equal ends are counted once, by the first interval that has them
            double gaps = 0.0;
            for (int cb = 0; cb <= K; cb += 64) {
                const int c = cb + lane;
                if (c <= K) {
                    const double p = c == 0 ? 0.0 : ivl[2 * (c - 1) + 1];
                    bool ok = p < 1.0;
                    double next = 1.0;
                    for (int k = 0; k < K; ++k) {
                        const double lo = ivl[2 * k], hi = ivl[2 * k + 1];
                        if (lo <= p && p < hi) ok = false;
                        if (lo > p && lo < next) next = lo;
                        if (c > 0 && k < c - 1 && hi == p) ok = false;
                    }
                    if (ok) gaps += next - p;
                }
            }
            for (int d = 32; d >= 1; d >>= 1) gaps += __shfl_xor(gaps, d, 64);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            acc += gaps * (0.5 * ev_cross(ax - rx, ay - ry, bx - rx, by - ry));
        }
    }
    if (lane == 0) wsum[w] = acc;
    __syncthreads();
    double r = 0.0;
    for (int k = 0; k < EV_WAVES; ++k) r += wsum[k];
    __syncthreads();
    return fmax(r, 0.0);
}

// ---- phase 3: matching, group and by-area unions, per-threshold records (evaluation.py:229-404) ---------------------------------
template <int MAXV>
__global__ __launch_bounds__(EV_THREADS) void ev_match_kernel(const int32_t *__restrict__ classes, const int32_t *__restrict__ counts,
                                                              const int32_t *__restrict__ gt_class, char *__restrict__ ws, ev_layout L,
                                                              ev_launch A, const int32_t *__restrict__ flags,
                                                              ubd_eval_record *__restrict__ per_image)
{
    __shared__ double s_ivl[EV_WAVES][2 * (EV_MAX_GT + EV_MAX_FOUND)];
    __shared__ double s_wsum[EV_WAVES];
    __shared__ double s_iou_g[EV_MAX_GT], s_iou_f[EV_MAX_FOUND];      // 1-1 pair IoU or 1-many group IoU; many-1 group IoU
    __shared__ int s_ngf[EV_MAX_GT], s_nfg[EV_MAX_FOUND], s_first[EV_MAX_GT];
    __shared__ unsigned char s_kind_g[EV_MAX_GT], s_kind_f[EV_MAX_FOUND];   // 0 none, 1 one-to-one, 2 one-to-many; 1 many-to-one
    __shared__ short s_list[EV_MAX_GT + EV_MAX_FOUND];
    __shared__ int s_m;

    const int li = blockIdx.x, img = A.img0 + li, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int G = A.gt0[li + 1] - A.gt0[li];
    const int flag = flags[img];
    const int cnt = counts[img];
    const int F = flag ? 0 : cnt;
    ubd_eval_record *rec = (ubd_eval_record *)(ws + L.off_rec) + (size_t)img * A.T;
    double *cm_img = (double *)(ws + L.off_cm) + (size_t)img * A.T * A.C * A.C;
    if (flag) {                                   // never score a truncated or malformed list: an all-zero record that carries the flag
        if (tid < A.T) {
            ubd_eval_record r;
            memset(&r, 0, sizeof(r));
            r.flags = flag; r.n_gt = G; r.n_found = cnt;
            rec[tid] = r;
            if (per_image) per_image[(size_t)img * A.T + tid] = r;
        }
        for (int k = tid; k < A.T * A.C * A.C; k += EV_THREADS) cm_img[k] = 0.0;
        return;
    }
    ev_image im;
    im.xy = (const double *)(ws + L.off_xy) + (size_t)img * L.P * (2 * MAXV);
    im.nv = (const int32_t *)(ws + L.off_nv) + (size_t)img * L.P;
    const double *tab = (const double *)(ws + L.off_tab) + (size_t)img * L.tab_stride;
    im.area_g = tab; im.area_f = tab + A.max_gt;
    im.inter = tab + A.max_gt + A.cap; im.iou = im.inter + (size_t)A.max_gt * A.cap;
    im.G = G; im.F = F; im.cap = A.cap; im.max_gt = A.max_gt;

    // adjacency counts (evaluation.py:235-239)
    for (int g = tid; g < G; g += EV_THREADS) {
        int c = 0, first = -1;
        for (int f = 0; f < F; ++f)
            if (im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU) { if (!c) first = f; ++c; }
        s_ngf[g] = c; s_first[g] = first;
    }
    for (int f = tid; f < F; f += EV_THREADS) {
        int c = 0;
        for (int g = 0; g < G; ++g) c += im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU;
        s_nfg[f] = c;
    }
    __syncthreads();
    // classes of correspondences (evaluation.py:241-260)
    for (int g = tid; g < G; g += EV_THREADS) {
        int kind = 0;
        double v = 0.0;
        if (s_ngf[g] == 1) {
            if (s_nfg[s_first[g]] == 1) { kind = 1; v = im.iou[(size_t)g * A.cap + s_first[g]]; }
        } else if (s_ngf[g] > 1) {
            kind = 2;
            for (int f = 0; f < F; ++f)
                if (im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU && s_nfg[f] != 1) kind = 0;
        }
        s_kind_g[g] = (unsigned char)kind; s_iou_g[g] = v;
    }
    for (int f = tid; f < F; f += EV_THREADS) {
        int kind = 0;
        if (s_nfg[f] > 1) {
            kind = 1;
            for (int g = 0; g < G; ++g)
                if (im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU && s_ngf[g] != 1) kind = 0;
        }
        s_kind_f[f] = (unsigned char)kind; s_iou_f[f] = 0.0;
    }
    __syncthreads();

    // by area (evaluation.py:389-404): union of all ground truths against union of all found quads
    for (int k = tid; k < G + F; k += EV_THREADS) s_list[k] = (short)(k < G ? k : A.max_gt + (k - G));
    __syncthreads();
    const double area_G = ev_union_area<MAXV>(im, s_list, G, s_ivl[w], s_wsum);
    const double area_F = ev_union_area<MAXV>(im, s_list + G, F, s_ivl[w], s_wsum);
    const double area_all = ev_union_area<MAXV>(im, s_list, G + F, s_ivl[w], s_wsum);
    const double inter_GF = fmin(fmax(area_G + area_F - area_all, 0.0), fmin(area_G, area_F));
    const double p_area = area_F > 0.0 ? inter_GF / area_F : 0.0;
    const double r_area = area_G > 0.0 ? inter_GF / area_G : 0.0;
    const double iou_area = ev_iou(area_G, area_F, inter_GF);
    __syncthreads();

    // group IoU (evaluation.py:379-387): the group's union against the single box, for 1-many then many-1
    for (int pass = 0; pass < 2; ++pass) {
        const int cnt_outer = pass == 0 ? G : F, cnt_inner = pass == 0 ? F : G;
        for (int o = 0; o < cnt_outer; ++o) {
            if ((pass == 0 ? s_kind_g[o] != 2 : s_kind_f[o] != 1)) continue;          // block-uniform
            if (w == 0) {                                                            // members of the group, in index order
                int m = 0;
                for (int b = 0; b < cnt_inner; b += 64) {
                    const int i = b + lane;
                    const bool adj = i < cnt_inner && (pass == 0 ? im.iou[(size_t)o * A.cap + i] : im.iou[(size_t)i * A.cap + o]) > EV_ADJ_IOU;
                    const unsigned long long mask = __ballot(adj);
                    if (adj) s_list[m + __popcll(mask & ((1ull << lane) - 1ull))] = (short)(pass == 0 ? A.max_gt + i : i);
                    m += __popcll(mask);
                }
                if (lane == 0) { s_list[m] = (short)(pass == 0 ? o : A.max_gt + o); s_m = m; }
            }
            __syncthreads();
            const int m = s_m;
            const double a_group = ev_union_area<MAXV>(im, s_list, m, s_ivl[w], s_wsum);
            const double a_all = ev_union_area<MAXV>(im, s_list, m + 1, s_ivl[w], s_wsum);
            const double a_box = pass == 0 ? im.area_g[o] : im.area_f[o];
            const double inter = fmin(fmax(a_group + a_box - a_all, 0.0), fmin(a_group, a_box));
            if (tid == 0) { if (pass == 0) s_iou_g[o] = ev_iou(a_group, a_box, inter); else s_iou_f[o] = ev_iou(a_group, a_box, inter); }
            __syncthreads();
        }
    }

    // one thread per threshold, in the reference's order: 1-1 pairs by ground truth, 1-many by ground truth, many-1 by found quad
    if (tid < A.T) {
        const double thr = A.thr[tid];
        const int C = A.C;
        double *cm = cm_img + (size_t)tid * C * C;
        for (int k = 0; k < C * C; ++k) cm[k] = 0.0;
        const int32_t *gcls = (C > 0) ? gt_class + A.gt0[li] : nullptr;
        const int32_t *fcls = (C > 0) ? classes + (size_t)img * A.cap : nullptr;
        int matched_gt = 0, matched_found = 0, o2o = 0, o2m = 0, m2o = 0, boxes = 0;
        double iou_sum = 0.0;
        for (int g = 0; g < G; ++g)
            if (s_kind_g[g] == 1 && s_iou_g[g] >= thr) {
                ++o2o; iou_sum += s_iou_g[g];
                if (C > 0) {
                    const int a = gcls[g], p = fcls[s_first[g]];
                    if (a >= 0 && a < C && p >= 0 && p < C) cm[a * C + p] += 1.0;
                }
            }
        matched_gt = matched_found = boxes = o2o;
        for (int g = 0; g < G; ++g)
            if (s_kind_g[g] == 2 && s_iou_g[g] >= thr) {
                ++matched_gt; ++o2m; ++boxes; matched_found += s_ngf[g]; iou_sum += s_iou_g[g];
                if (C > 0) {                                    // evaluation.py:346-354: weights inter / sum(inter)
                    double tot = 0.0;
                    for (int f = 0; f < F; ++f)
                        if (im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU) tot += im.inter[(size_t)g * A.cap + f];
                    const int a = gcls[g];
                    for (int f = 0; f < F; ++f)
                        if (im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU) {
                            const int p = fcls[f];
                            if (a >= 0 && a < C && p >= 0 && p < C) cm[a * C + p] += im.inter[(size_t)g * A.cap + f] / tot;
                        }
                }
            }
        for (int f = 0; f < F; ++f)
            if (s_kind_f[f] == 1 && s_iou_f[f] >= thr) {
                matched_gt += s_nfg[f]; m2o += s_nfg[f]; ++matched_found; ++boxes; iou_sum += s_iou_f[f];
                if (C > 0) {
                    const int p = fcls[f];
                    for (int g = 0; g < G; ++g)
                        if (im.iou[(size_t)g * A.cap + f] > EV_ADJ_IOU) {
                            const int a = gcls[g];
                            if (a >= 0 && a < C && p >= 0 && p < C) cm[a * C + p] += 1.0;
                        }
                }
            }
        ubd_eval_record r;
        r.tp = matched_gt; r.fp = F - matched_found; r.fn = G - matched_gt;
        r.one_to_one = o2o; r.one_to_many = o2m; r.many_to_one = m2o; r.matched_boxes_count = boxes;
        r.detection_rate = iou_area > thr ? 1 : 0;              // strict, evaluation.py:322
        r.n_gt = G; r.n_found = F; r.flags = 0; r.reserved = 0;
        r.iou_sum = iou_sum; r.precision_by_area = p_area; r.recall_by_area = r_area; r.iou_by_area = iou_area;
        rec[tid] = r;
        if (per_image) per_image[(size_t)img * A.T + tid] = r;
    }
}

// ---- phase 4: records -> accumulator, images in order, one block -----------------------------------------------------------------
__global__ __launch_bounds__(EV_THREADS) void ev_accumulate_kernel(const char *__restrict__ ws, ev_layout L, ev_launch A, void *accumulator)
{
    int64_t *ai = (int64_t *)accumulator;
    double *ad = (double *)accumulator;
    const int tid = threadIdx.x, T = A.T, C = A.C;
    const ubd_eval_record *rec = (const ubd_eval_record *)(ws + L.off_rec);
    if (tid == 0) {
        for (int i = A.img0; i < A.img0 + A.m; ++i) {
            const ubd_eval_record &r = rec[(size_t)i * T];
            if (r.flags) { ai[1] += 1; continue; }
            ai[0] += 1;
            ad[2] += r.precision_by_area; ad[3] += r.recall_by_area; ad[4] += r.iou_by_area;
        }
    }
    if (tid >= 64 && tid < 64 + T) {
        const int t = tid - 64;
        int64_t *pi = ai + EV_ACC_HEAD + (size_t)t * EV_ACC_PER_T;
        double *pd = ad + EV_ACC_HEAD + (size_t)t * EV_ACC_PER_T;
        for (int i = A.img0; i < A.img0 + A.m; ++i) {
            const ubd_eval_record &r = rec[(size_t)i * T + t];
            if (r.flags) continue;
            pi[0] += r.tp; pi[1] += r.fp; pi[2] += r.fn; pi[3] += r.one_to_one; pi[4] += r.one_to_many; pi[5] += r.many_to_one;
            pi[6] += r.matched_boxes_count; pi[7] += r.detection_rate;
            pd[8] += r.iou_sum;
        }
    }
    const double *cm = (const double *)(ws + L.off_cm);
    double *acm = ad + EV_ACC_HEAD + (size_t)T * EV_ACC_PER_T;
    for (int k = tid; k < T * C * C; k += EV_THREADS) {
        double s = acm[k];
        for (int i = A.img0; i < A.img0 + A.m; ++i) s += cm[(size_t)i * T * C * C + k];
        acm[k] = s;
    }
}

extern "C" size_t ubd_evaluate_accumulator_bytes(int n_thresholds, int n_classes)
{
    if (n_thresholds < 1 || n_thresholds > EV_MAX_T || n_classes < 0 || n_classes > UBD_MAX_CLASSES) return 0;
    return ((size_t)EV_ACC_HEAD + (size_t)EV_ACC_PER_T * n_thresholds + (size_t)n_thresholds * n_classes * n_classes) * 8;
}

static_assert(EV_MAX_V % EV_WAVES == 0 && UBD_POLY_MAX_VERTS % EV_WAVES == 0, "an edge must land in the same wave for either slot size");

static size_t ev_workspace_bytes(int n, int max_gt, int cap, int n_thresholds, int n_classes, int maxv)
{
    if (n < 1 || max_gt < 1 || max_gt > EV_MAX_GT || cap < 1 || cap > EV_MAX_FOUND || n_thresholds < 1 || n_thresholds > EV_MAX_T ||
        n_classes < 0 || n_classes > UBD_MAX_CLASSES)
        return 0;
    ev_layout L;
    ev_layout_compute(n, max_gt, cap, n_thresholds, n_classes, maxv, &L);
    return L.total + (size_t)n * sizeof(int32_t) + 256;          // + the per-image flags
}

extern "C" size_t ubd_evaluate_workspace_bytes(int n, int max_gt, int cap, int n_thresholds, int n_classes)
{
    return ev_workspace_bytes(n, max_gt, cap, n_thresholds, n_classes, EV_MAX_V);
}

extern "C" size_t ubd_evaluate_polygons_workspace_bytes(int n, int max_gt, int cap, int n_thresholds, int n_classes, int max_verts)
{
    if (max_verts < 3 || max_verts > UBD_POLY_MAX_VERTS) return 0;
    return ev_workspace_bytes(n, max_gt, cap, n_thresholds, n_classes, UBD_POLY_MAX_VERTS);
}

static int ev_tables_layout(const char *who, int n, int max_gt, int cap, int n_thresholds, int n_classes, int maxv, int64_t *offset_bytes,
                            int64_t *stride_doubles)
{
    UBD_REQUIRE(offset_bytes && stride_doubles, "%s: null argument", who);
    UBD_REQUIRE(ev_workspace_bytes(n, max_gt, cap, n_thresholds, n_classes, maxv) != 0, "%s: bad sizes", who);
    ev_layout L;
    ev_layout_compute(n, max_gt, cap, n_thresholds, n_classes, maxv, &L);
    *offset_bytes = (int64_t)L.off_tab;
    *stride_doubles = (int64_t)L.tab_stride;
    return 0;
}

extern "C" int ubd_evaluate_tables_layout(int n, int max_gt, int cap, int n_thresholds, int n_classes, int64_t *offset_bytes,
                                          int64_t *stride_doubles)
{
    return ev_tables_layout("ubd_evaluate_tables_layout", n, max_gt, cap, n_thresholds, n_classes, EV_MAX_V, offset_bytes, stride_doubles);
}

extern "C" int ubd_evaluate_polygons_tables_layout(int n, int max_gt, int cap, int n_thresholds, int n_classes, int max_verts,
                                                   int64_t *offset_bytes, int64_t *stride_doubles)
{
    UBD_REQUIRE(max_verts >= 3 && max_verts <= UBD_POLY_MAX_VERTS, "ubd_evaluate_polygons_tables_layout: max_verts must be 3..%d, got %d",
                UBD_POLY_MAX_VERTS, max_verts);
    return ev_tables_layout("ubd_evaluate_polygons_tables_layout", n, max_gt, cap, n_thresholds, n_classes, UBD_POLY_MAX_VERTS, offset_bytes,
                            stride_doubles);
}

template <int MAXV>
static int ev_evaluate(const char *who, const int32_t *quads, const int32_t *classes, const int32_t *counts, int n, int cap,
                       const double *scales, const double *gt_xy, int n_gt_vertices, const int32_t *gt_first,
                       const int32_t *gt_class, const int32_t *gt_image_first, int max_gt, const double *thresholds,
                       int n_thresholds, int n_classes, int max_verts, ubd_eval_record *per_image, void *accumulator, void *workspace,
                       size_t workspace_bytes, void *stream)
{
    UBD_REQUIRE(quads && counts && gt_xy && gt_first && gt_image_first && thresholds, "%s: null argument", who);
    UBD_REQUIRE(accumulator, "%s: null accumulator", who);
    UBD_REQUIRE(workspace, "%s: null workspace", who);
    UBD_REQUIRE(n >= 1, "%s: n must be >= 1, got %d", who, n);
    UBD_REQUIRE(cap >= 1 && cap <= EV_MAX_FOUND, "%s: cap must be 1..%d, got %d", who, EV_MAX_FOUND, cap);
    UBD_REQUIRE(n_thresholds >= 1 && n_thresholds <= EV_MAX_T, "%s: n_thresholds must be 1..%d, got %d", who, EV_MAX_T, n_thresholds);
    UBD_REQUIRE(n_classes >= 0 && n_classes <= UBD_MAX_CLASSES, "%s: n_classes must be 0..%d, got %d", who, UBD_MAX_CLASSES, n_classes);
    UBD_REQUIRE(n_classes == 0 || (classes && gt_class), "%s: classes and gt_class are required when n_classes > 0", who);
    UBD_REQUIRE(max_gt >= 1 && max_gt <= EV_MAX_GT, "%s: max_gt must be 1..%d, got %d", who, EV_MAX_GT, max_gt);
    UBD_REQUIRE(max_verts >= 3 && max_verts <= MAXV, "%s: max_verts must be 3..%d, got %d", who, MAXV, max_verts);
    UBD_REQUIRE(n_gt_vertices >= 0, "%s: n_gt_vertices is negative", who);
    UBD_REQUIRE(gt_image_first[0] >= 0, "%s: gt_image_first[0] is negative", who);
    for (int i = 0; i < n; ++i) {
        const int64_t g = (int64_t)gt_image_first[i + 1] - gt_image_first[i];
        UBD_REQUIRE(g >= 0, "%s: gt_image_first decreases at image %d", who, i);
        UBD_REQUIRE(g <= EV_MAX_GT, "%s: image %d has %lld ground-truth polygons, the limit is %d", who, i, (long long)g, EV_MAX_GT);
        UBD_REQUIRE(g <= max_gt, "%s: image %d has %lld ground-truth polygons, max_gt is %d", who, i, (long long)g, max_gt);
    }
    for (int t = 0; t < n_thresholds; ++t)
        UBD_REQUIRE(thresholds[t] == thresholds[t], "%s: threshold %d is not a number", who, t);
    ev_layout L;
    ev_layout_compute(n, max_gt, cap, n_thresholds, n_classes, MAXV, &L);
    const size_t need = ev_workspace_bytes(n, max_gt, cap, n_thresholds, n_classes, MAXV);
    UBD_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    char *ws = (char *)workspace;
    int32_t *flags = (int32_t *)(ws + L.total);
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += EV_MAX_IMGS) {
        ev_launch A{};
        A.m = std::min(EV_MAX_IMGS, n - i0);
        A.img0 = i0; A.max_gt = max_gt; A.cap = cap; A.T = n_thresholds; A.C = n_classes; A.max_verts = max_verts;
        A.n_gt_verts = n_gt_vertices;
        int gmax = 1;
        for (int k = 0; k <= A.m; ++k) A.gt0[k] = gt_image_first[i0 + k];
        for (int k = 0; k < A.m; ++k) gmax = std::max(gmax, A.gt0[k + 1] - A.gt0[k]);
        for (int t = 0; t < n_thresholds; ++t) A.thr[t] = thresholds[t];
        hipLaunchKernelGGL(ev_prepare_kernel<MAXV>, dim3(A.m), dim3(EV_THREADS), 0, st, quads, counts, scales, gt_xy, gt_first, ws, L, A, flags);
        hipLaunchKernelGGL(ev_tables_kernel<MAXV>, dim3(gmax, A.m), dim3(64), 0, st, counts, ws, L, A);
        hipLaunchKernelGGL(ev_match_kernel<MAXV>, dim3(A.m), dim3(EV_THREADS), 0, st, classes, counts, gt_class, ws, L, A, (const int32_t *)flags, per_image);
        hipLaunchKernelGGL(ev_accumulate_kernel, dim3(1), dim3(EV_THREADS), 0, st, (const char *)ws, L, A, accumulator);
        UBD_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int ubd_evaluate_objects(const int32_t *quads, const int32_t *classes, const int32_t *counts, int n, int cap,
                                    const double *scales, const double *gt_xy, int n_gt_vertices, const int32_t *gt_first,
                                    const int32_t *gt_class, const int32_t *gt_image_first, int max_gt, const double *thresholds,
                                    int n_thresholds, int n_classes, ubd_eval_record *per_image, void *accumulator, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    return ev_evaluate<EV_MAX_V>("ubd_evaluate_objects", quads, classes, counts, n, cap, scales, gt_xy, n_gt_vertices, gt_first, gt_class,
                                 gt_image_first, max_gt, thresholds, n_thresholds, n_classes, EV_MAX_V, per_image, accumulator, workspace,
                                 workspace_bytes, stream);
}

extern "C" int ubd_evaluate_polygons(const int32_t *quads, const int32_t *classes, const int32_t *counts, int n, int cap,
                                     const double *scales, const double *gt_xy, int n_gt_vertices, const int32_t *gt_first,
                                     const int32_t *gt_class, const int32_t *gt_image_first, int max_gt, const double *thresholds,
                                     int n_thresholds, int n_classes, int max_verts, ubd_eval_record *per_image, void *accumulator,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    UBD_REQUIRE(max_verts >= 3 && max_verts <= UBD_POLY_MAX_VERTS, "ubd_evaluate_polygons: max_verts must be 3..%d, got %d",
                UBD_POLY_MAX_VERTS, max_verts);
    return ev_evaluate<UBD_POLY_MAX_VERTS>("ubd_evaluate_polygons", quads, classes, counts, n, cap, scales, gt_xy, n_gt_vertices, gt_first,
                                           gt_class, gt_image_first, max_gt, thresholds, n_thresholds, n_classes, max_verts, per_image,
                                           accumulator, workspace, workspace_bytes, stream);
}
