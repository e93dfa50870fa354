// Per-object detection scores and the ranked detection records of an evaluation epoch.  No reference counterpart: the reference
// has no confidence of a found object and no average precision (include/ubd.h states the definitions).
//
// ubd_score_objects: the score of a found object is the mean detection probability over its REGION, the map pixels
// ubd_build_label_maps would paint for its quad at `scale`: rq_proper_round(quad / scale) (raster_round.h), then Pillow's polygon
// rule (raster_fill.h), clipped to the map.  The region is the found box, not the component's filled contour -- a stated deviation:
// a thin diagonal object scores lower than its own pixels would.  The arithmetic is fixed so that any parallelisation gives the
// same bits: p = 1 / (1 + expf(-x)) in fp32 (NaN counts as 0), q = rint(p * 2^24) as an integer, the q summed in 64-bit integers,
// score = (float)((double)sum / (2^24 * (double)count)).  One block per (image, slot); a lane answers a run of up to 32 pixels of a
// row from one scan-line evaluation (rq_covers_run) and adds the logits of the set bits; integer sums commute, so no order is kept.
//
// ubd_rank_detections: COCO's greedy matching per image at every IoU threshold at once, appended to an epoch buffer in image order.
// Two launches: one block per image ranks, matches and writes its records behind the records of the earlier images (every block
// adds up the earlier images' counts itself and reads the header's record count, which this launch does not write); a second
// one-block launch then moves the header on.  No atomics on global memory: the same calls give the same bytes.
#include "common.h"
#include "raster_fill.h"
#include "raster_round.h"

#define SC_THREADS 256
#define SC_RUN 32

__global__ __launch_bounds__(SC_THREADS) void score_objects_kernel(const float *__restrict__ logits, int pixel_stride,
                                                                   const int *__restrict__ quads, const int *__restrict__ counts,
                                                                   int map_h, int map_w, int cap, int scale, float *__restrict__ scores)
{
    __shared__ long long s_sum[SC_THREADS / 64];
    __shared__ int s_cnt[SC_THREADS / 64];
    const int img = blockIdx.x / cap, o = blockIdx.x - img * cap, tid = threadIdx.x;
    int cnt = counts[img];
    cnt = cnt < cap ? cnt : cap;
    if (o >= cnt) {                                                 // block-uniform: the whole tensor is defined
        if (tid == 0) scores[blockIdx.x] = 0.f;
        return;
    }
    double bbox[8];
    int pts[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bbox[k] = (double)quads[(size_t)blockIdx.x * 8 + k];
    rq_proper_round(bbox, scale, pts);
    // no covered pixel lies outside the row / column extent of the four corners (tests/test_raster_fill_host.py)
    const int x0 = max(min(min(pts[0], pts[2]), min(pts[4], pts[6])), 0), x1 = min(max(max(pts[0], pts[2]), max(pts[4], pts[6])), map_w - 1);
    const int y0 = max(min(min(pts[1], pts[3]), min(pts[5], pts[7])), 0), y1 = min(max(max(pts[1], pts[3]), max(pts[5], pts[7])), map_h - 1);
    long long sum = 0;
    int n_px = 0;
    if (x0 <= x1 && y0 <= y1) {
        const int runs = (x1 - x0) / SC_RUN + 1, items = (y1 - y0 + 1) * runs;      // < 32768 * 1024
        const float *base = logits + (size_t)img * map_h * map_w * pixel_stride;
        for (int it = tid; it < items; it += SC_THREADS) {
            const int row = it / runs, py = y0 + row, px = x0 + (it - row * runs) * SC_RUN;
            unsigned bits = rq_covers_run(pts, px, min(SC_RUN, x1 - px + 1), py, map_h);
            n_px += __popc(bits);
            const float *line = base + ((size_t)py * map_w + px) * pixel_stride;
            while (bits) {
                const int k = __ffs(bits) - 1;
                bits &= bits - 1u;
                const float x = line[(size_t)k * pixel_stride];
                float p = 1.0f / (1.0f + expf(-x));
                if (!(p == p)) p = 0.f;
                sum += (long long)(uint32_t)rintf(p * 16777216.0f);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        n_px += __shfl_xor(n_px, d, 64);
    }
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sum; s_cnt[tid >> 6] = n_px; }
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
        int count = 0;
#pragma unroll
        for (int w = 0; w < SC_THREADS / 64; ++w) { total += s_sum[w]; count += s_cnt[w]; }
        scores[blockIdx.x] = count > 0 ? (float)((double)total / (16777216.0 * (double)count)) : 0.f;
    }
}

extern "C" int ubd_score_objects(const float *logits, int pixel_stride, const int32_t *quads, const int32_t *counts, int n, int map_h,
                                 int map_w, int cap, int scale, float *scores, void *stream)
{
    const char *fn = "ubd_score_objects";
    UBD_REQUIRE(logits && quads && counts && scores, "%s: null argument", fn);
    UBD_REQUIRE(n > 0 && map_h > 0 && map_w > 0 && cap > 0 && scale > 0 && pixel_stride > 0,
                "%s: n, map_h, map_w, cap, scale and pixel_stride must be positive", fn);
    UBD_REQUIRE(map_h < 32768 && map_w < 32768, "%s: map sides must stay below 32768, got %d x %d", fn, map_h, map_w);
    UBD_REQUIRE((long long)n * map_h * map_w < (1ll << 31), "%s: n * map_h * map_w must stay below 2^31", fn);
    UBD_REQUIRE((long long)n * cap < (1ll << 31), "%s: n * cap must stay below 2^31", fn);
    hipLaunchKernelGGL(score_objects_kernel, dim3((unsigned)(n * cap)), dim3(SC_THREADS), 0, (hipStream_t)stream, logits, pixel_stride, quads,
                       counts, map_h, map_w, cap, scale, scores);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ ubd_rank_detections
#define RK_THREADS 256
#define RK_GROUP 16                       // lanes per threshold: UBD_EVAL_MAX_THRESHOLDS groups make the block
#define RK_HEADER 8                       // int64 slots before the records
static_assert(RK_GROUP * UBD_EVAL_MAX_THRESHOLDS == RK_THREADS, "one group of lanes per threshold");
static_assert(UBD_EVAL_MAX_FOUND <= RK_THREADS && UBD_EVAL_MAX_GT <= RK_THREADS, "one lane per detection / ground truth");

struct rk_record { float score; uint32_t tp_mask; };
struct rk_thresholds { double t[UBD_EVAL_MAX_THRESHOLDS]; };
static_assert(sizeof(rk_record) == 8, "record layout");

// an image that is not ranked: its list was truncated, or it has more ground truth than an IoU table holds
__device__ __forceinline__ bool rk_flagged(int count, int gt, int cap) { return count > cap || gt > UBD_EVAL_MAX_GT; }

// does detection a come before detection b?  descending score, ties to the lower index, NaN last
__device__ __forceinline__ bool rk_before(float sa, int a, float sb, int b)
{
    const bool na = !(sa == sa), nb = !(sb == sb);
    if (na != nb) return nb;
    if (!na && sa != sb) return sa > sb;
    return a < b;
}

__global__ __launch_bounds__(RK_THREADS) void rank_detections_kernel(const float *__restrict__ scores, const int *__restrict__ counts, int cap,
                                                                     const double *__restrict__ iou, long long image_stride,
                                                                     const int *__restrict__ gt_counts, rk_thresholds thr, int n_thr,
                                                                     const long long *__restrict__ header, rk_record *__restrict__ records,
                                                                     long long capacity)
{
    __shared__ float s_score[UBD_EVAL_MAX_FOUND];
    __shared__ int s_order[UBD_EVAL_MAX_FOUND];
    __shared__ unsigned s_mask[UBD_EVAL_MAX_FOUND];
    __shared__ double s_col[UBD_EVAL_MAX_GT];
    __shared__ unsigned char s_taken[UBD_EVAL_MAX_THRESHOLDS][UBD_EVAL_MAX_GT];
    __shared__ long long s_part[RK_THREADS / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int raw_count = counts[img], raw_gt = gt_counts[img];
    if (rk_flagged(raw_count, raw_gt, cap)) return;                 // block-uniform
    const int cnt = max(raw_count, 0), n_gt = max(raw_gt, 0);
    if (cnt == 0) return;
    // where this image's records go: behind the records of the buffer and those of the earlier images of this call
    long long before = 0;
    for (int i = tid; i < img; i += RK_THREADS) {
        const int c = counts[i];
        if (!rk_flagged(c, gt_counts[i], cap)) before += max(c, 0);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = before;
    if (tid < cnt) { s_score[tid] = scores[(size_t)img * cap + tid]; s_mask[tid] = 0u; }
    for (int k = tid; k < UBD_EVAL_MAX_THRESHOLDS * UBD_EVAL_MAX_GT; k += RK_THREADS) (&s_taken[0][0])[k] = 0;
    __syncthreads();
    long long first = header[0];
#pragma unroll
    for (int w = 0; w < RK_THREADS / 64; ++w) first += s_part[w];
    if (tid < cnt) {                                                // rank sort: the order is total, every rank is taken once
        const float mine = s_score[tid];
        int rank = 0;
        for (int j = 0; j < cnt; ++j) rank += (j != tid && rk_before(s_score[j], j, mine, tid)) ? 1 : 0;
        s_order[rank] = tid;
    }
    __syncthreads();
    const int group = tid / RK_GROUP, lane = tid - group * RK_GROUP;
    const double *table = iou + (size_t)img * image_stride;
    for (int r = 0; r < cnt; ++r) {                                 // greedy: one detection after the other, every threshold beside the others
        const int f = s_order[r];
        if (tid < n_gt) s_col[tid] = table[(size_t)tid * cap + f];
        __syncthreads();
        if (group < n_thr) {
            double best = 0.0;
            int best_g = -1;
            for (int g = lane; g < n_gt; g += RK_GROUP) {           // ascending g: a strict comparison keeps the lowest of equals
                const double v = s_col[g];
                if (!s_taken[group][g] && v == v && (best_g < 0 || v > best)) { best = v; best_g = g; }
            }
#pragma unroll
            for (int d = RK_GROUP / 2; d > 0; d >>= 1) {
                const double ov = __shfl_xor(best, d, RK_GROUP);
                const int og = __shfl_xor(best_g, d, RK_GROUP);
                if (og >= 0 && (best_g < 0 || ov > best || (ov == best && og < best_g))) { best = ov; best_g = og; }
            }
            if (lane == 0 && best_g >= 0 && best >= thr.t[group]) {
                s_taken[group][best_g] = 1;
                atomicOr(&s_mask[r], 1u << group);
            }
        }
        __syncthreads();
    }
    if (tid < cnt && first + tid < capacity) {
        rk_record rec;
        rec.score = s_score[s_order[tid]];
        rec.tp_mask = s_mask[tid];
        records[first + tid] = rec;
    }
}

// after the records: [0] written, [1] dropped, [2] ground truths of the scored images, [3] images scored, [4] images flagged
__global__ __launch_bounds__(RK_THREADS) void rank_header_kernel(const int *__restrict__ counts, int n, int cap, const int *__restrict__ gt_counts,
                                                                 long long *__restrict__ header, long long capacity)
{
    __shared__ long long s_part[RK_THREADS / 64][4];
    const int tid = threadIdx.x;
    long long v[4] = {0, 0, 0, 0};                                  // records, ground truths, scored, flagged
    for (int i = tid; i < n; i += RK_THREADS) {
        const int c = counts[i], g = gt_counts[i];
        if (rk_flagged(c, g, cap)) v[3] += 1;
        else { v[0] += max(c, 0); v[1] += max(g, 0); v[2] += 1; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if ((tid & 63) == 0) s_part[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid == 0) {
        long long t[4] = {0, 0, 0, 0};
        for (int w = 0; w < RK_THREADS / 64; ++w)
            for (int k = 0; k < 4; ++k) t[k] += s_part[w][k];
        const long long end = header[0] + t[0], written = end < capacity ? end : capacity;
        header[0] = written;
        header[1] += end - written;
        header[2] += t[1];
        header[3] += t[2];
        header[4] += t[3];
    }
}

extern "C" size_t ubd_rank_buffer_bytes(int64_t capacity)
{
    if (capacity < 1 || capacity > (int64_t)1 << 56) return 0;
    return (size_t)(RK_HEADER + capacity) * 8;
}

extern "C" int ubd_rank_detections(const float *scores, const int32_t *counts, int n, int cap, const double *iou,
                                   int64_t image_stride_doubles, const int32_t *gt_counts, const double *thresholds, int n_thresholds,
                                   void *rank_buffer, int64_t capacity, void *stream)
{
    const char *fn = "ubd_rank_detections";
    UBD_REQUIRE(scores && counts && iou && gt_counts && thresholds && rank_buffer, "%s: null argument", fn);
    UBD_REQUIRE(n > 0, "%s: n must be positive, got %d", fn, n);
    UBD_REQUIRE(cap > 0 && cap <= UBD_EVAL_MAX_FOUND, "%s: cap must be 1..%d, got %d", fn, UBD_EVAL_MAX_FOUND, cap);
    UBD_REQUIRE(n_thresholds > 0 && n_thresholds <= UBD_EVAL_MAX_THRESHOLDS, "%s: n_thresholds must be 1..%d, got %d", fn,
                UBD_EVAL_MAX_THRESHOLDS, n_thresholds);
    UBD_REQUIRE(image_stride_doubles > 0, "%s: image_stride_doubles must be positive", fn);
    UBD_REQUIRE(ubd_rank_buffer_bytes(capacity) != 0, "%s: capacity must be positive", fn);
    UBD_REQUIRE(((uintptr_t)rank_buffer & 7) == 0 && ((uintptr_t)iou & 7) == 0, "%s: misaligned argument", fn);
    rk_thresholds thr;
    for (int j = 0; j < UBD_EVAL_MAX_THRESHOLDS; ++j) thr.t[j] = j < n_thresholds ? thresholds[j] : 0.0;
    long long *header = (long long *)rank_buffer;
    hipLaunchKernelGGL(rank_detections_kernel, dim3((unsigned)n), dim3(RK_THREADS), 0, (hipStream_t)stream, scores, counts, cap, iou,
                       (long long)image_stride_doubles, gt_counts, thr, n_thresholds, (const long long *)header,
                       (rk_record *)(header + RK_HEADER), (long long)capacity);
    UBD_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(rank_header_kernel, dim3(1), dim3(RK_THREADS), 0, (hipStream_t)stream, counts, n, cap, gt_counts, header, (long long)capacity);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
