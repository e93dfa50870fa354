// Visualisations on device: the four overlays of Visualizer.compute_visualizations (semantic_segmentation/visualizations.py:20-151)
// for a whole batch in one pass over the image pixels.
//
// Every overlay is Visualizer.draw_segmentation_map (:138-151), Image.composite(Image.blend(image, solid(color), 0.5), image, mask):
// for 8-bit images and a 0 / 255 mask that is, per channel, out = (in + color) >> 1 where the mask is set and out = in elsewhere
// (tests/visualization_oracle.py holds the Pillow calls beside this closed form).  Masks at map resolution reach image size as
// Image.resize(NEAREST) does for an integer ratio s: mask[y / s][x / s].  The found boxes are filled at image resolution with
// ImageDraw.polygon's rule (raster_fill.h), tested straight on the int32 quads ubd_postprocess left in device memory.
//
// One lane takes a run of four adjacent pixels of a row: 4 or 12 bytes in, and 12 bytes (three dwords) out per overlay; with s = 4
// the run reads one map entry per mask.  A block is a tile of 256 runs of one image (as wide as the row allows, at most 64 runs);
// it stages the image's quads in LDS together with their row / column extents, 64 at a time, and a lane runs the scan-line rule
// only for quads whose extent meets its run.  Dword accesses where the address is a multiple of 4, bytes elsewhere (rows of
// width 5 have a 15-byte pitch: the alignment changes from row to row) and in the tail of a row.
#include "common.h"
#include "raster_fill.h"

#define VZ_THREADS 256
#define VZ_RUN 4              // pixels per lane
#define VZ_QCHUNK 64          // quads staged per round

struct vz_args {
    const void *images;
    const int32_t *gt_labels, *binary_map, *quads, *counts;
    const int8_t *cls_mask;
    uint8_t *out_gt, *out_seg_map, *out_postprocessed, *out_classification_gt;
    int in_f32, mobilenet, height, width, channels, map_w, ratio, cap;
    int tile_w_log2;          // a tile is (1 << tile_w_log2) runs wide and VZ_THREADS >> tile_w_log2 rows high
    int tiles_x, tiles_y;
};

// denorm + astype(uint8) of a float pixel: product and sum rounded separately, clamp to [0, 255] (NaN -> 0), truncate
__device__ __forceinline__ unsigned vz_to_u8(float x, int mobilenet)
{
    if (mobilenet) x = __fadd_rn(__fmul_rn(x, 127.5f), 127.5f);
    return (unsigned)(int)fminf(fmaxf(x, 0.f), 255.f);
}

// one overlay of a run: px[k][c] blended with green where bit k of `green` is set, with red where bit k of `red` is set
__device__ __forceinline__ void vz_emit(uint8_t *out, size_t byte_off, const unsigned (&px)[VZ_RUN][3], unsigned green, unsigned red, int npx)
{
    unsigned b[VZ_RUN * 3];
#pragma unroll
    for (int k = 0; k < VZ_RUN; ++k) {
        const bool g = (green >> k) & 1u, r = (red >> k) & 1u;
        b[3 * k + 0] = g ? px[k][0] >> 1 : r ? (px[k][0] + 255u) >> 1 : px[k][0];
        b[3 * k + 1] = g ? (px[k][1] + 255u) >> 1 : r ? px[k][1] >> 1 : px[k][1];
        b[3 * k + 2] = (g || r) ? px[k][2] >> 1 : px[k][2];
    }
    uint8_t *dst = out + byte_off;
    if (npx == VZ_RUN && ((size_t)dst & 3) == 0) {
        unsigned *d = (unsigned *)dst;
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < VZ_RUN; ++k)
            if (k < npx) { dst[3 * k] = (uint8_t)b[3 * k]; dst[3 * k + 1] = (uint8_t)b[3 * k + 1]; dst[3 * k + 2] = (uint8_t)b[3 * k + 2]; }
    }
}

__global__ __launch_bounds__(VZ_THREADS) void visualize_kernel(const vz_args a)
{
    __shared__ int s_pts[VZ_QCHUNK][8];
    __shared__ int s_ext[VZ_QCHUNK][4];       // xmin, xmax, ymin, ymax of the corners: the fill never leaves them

    // block -> (image, tile); all of it wave-uniform
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    const unsigned img = blockIdx.x / tiles, t = blockIdx.x - img * tiles;
    const unsigned tyi = t / (unsigned)a.tiles_x, txi = t - tyi * (unsigned)a.tiles_x;
    const int tile_w = 1 << a.tile_w_log2, tile_h = VZ_THREADS >> a.tile_w_log2;
    const int tid = (int)threadIdx.x;
    const int y = (int)tyi * tile_h + (tid >> a.tile_w_log2);
    const int x0 = ((int)txi * tile_w + (tid & (tile_w - 1))) * VZ_RUN;
    const bool live = y < a.height && x0 < a.width;
    const int npx = live ? min(VZ_RUN, a.width - x0) : 0;
    const size_t pix = ((size_t)img * a.height + (size_t)(live ? y : 0)) * a.width + (size_t)(live ? x0 : 0);

    // ---- the run's pixels as RGB
    unsigned px[VZ_RUN][3];
#pragma unroll
    for (int k = 0; k < VZ_RUN; ++k) px[k][0] = px[k][1] = px[k][2] = 0u;
    if (live) {
        const int nb = a.channels * VZ_RUN;                  // values of a full run
        unsigned v[VZ_RUN * 3];
        if (a.in_f32) {
            const float *src = (const float *)a.images + pix * a.channels;
            if (npx == VZ_RUN && ((size_t)src & 15) == 0) {
                const float4 f0 = ((const float4 *)src)[0];
                v[0] = vz_to_u8(f0.x, a.mobilenet); v[1] = vz_to_u8(f0.y, a.mobilenet); v[2] = vz_to_u8(f0.z, a.mobilenet); v[3] = vz_to_u8(f0.w, a.mobilenet);
                if (a.channels == 3) {
                    const float4 f1 = ((const float4 *)src)[1], f2 = ((const float4 *)src)[2];
                    v[4] = vz_to_u8(f1.x, a.mobilenet); v[5] = vz_to_u8(f1.y, a.mobilenet); v[6] = vz_to_u8(f1.z, a.mobilenet); v[7] = vz_to_u8(f1.w, a.mobilenet);
                    v[8] = vz_to_u8(f2.x, a.mobilenet); v[9] = vz_to_u8(f2.y, a.mobilenet); v[10] = vz_to_u8(f2.z, a.mobilenet); v[11] = vz_to_u8(f2.w, a.mobilenet);
                }
            } else {
#pragma unroll
                for (int j = 0; j < VZ_RUN * 3; ++j) v[j] = j < npx * a.channels ? vz_to_u8(src[j], a.mobilenet) : 0u;
            }
        } else {
            const uint8_t *src = (const uint8_t *)a.images + pix * a.channels;
            if (npx == VZ_RUN && ((size_t)src & 3) == 0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (4 * j < nb) {
                        const unsigned w = ((const unsigned *)src)[j];
                        v[4 * j] = w & 255u; v[4 * j + 1] = (w >> 8) & 255u; v[4 * j + 2] = (w >> 16) & 255u; v[4 * j + 3] = w >> 24;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < VZ_RUN * 3; ++j) v[j] = j < npx * a.channels ? (unsigned)src[j] : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < VZ_RUN; ++k) {
            if (a.channels == 3) { px[k][0] = v[3 * k]; px[k][1] = v[3 * k + 1]; px[k][2] = v[3 * k + 2]; }
            else px[k][0] = px[k][1] = px[k][2] = v[k];      // grey -> RGB: the channel three times
        }
    }

    // ---- the masks at map resolution: entry (y / s, x / s)
    unsigned m_gt = 0u, m_seg = 0u, m_ok = 0u, m_bad = 0u;
    const bool want_gt = a.out_gt != nullptr, want_seg = a.out_seg_map != nullptr, want_cls = a.out_classification_gt != nullptr;
    if (live && (want_gt || want_seg || want_cls)) {
        const int s = a.ratio;
        const int my = y / s;
        int mx = x0 / s, r = x0 - mx * s;
        const size_t row = ((size_t)img * (size_t)(a.height / s) + (size_t)my) * a.map_w;
        int gt = 0, seg = 0, cls = 0;
#pragma unroll
        for (int k = 0; k < VZ_RUN; ++k) {
            if (k < npx) {
                if (k == 0 || r == 0) {                      // a new map entry
                    if (want_gt) gt = a.gt_labels[row + mx];
                    if (want_seg) seg = a.binary_map[row + mx];
                    if (want_cls) cls = a.cls_mask[row + mx];
                }
                m_gt |= (gt > 0 ? 1u : 0u) << k;
                m_seg |= (seg > 0 ? 1u : 0u) << k;
                m_ok |= (cls == 1 ? 1u : 0u) << k;
                m_bad |= (cls == -1 ? 1u : 0u) << k;
                if (++r == s) { r = 0; ++mx; }
            }
        }
    }

    // ---- the found boxes at image resolution (every thread of the block walks the rounds: they hold barriers)
    unsigned m_box = 0u;
    if (a.out_postprocessed != nullptr) {
        int cnt = a.counts[img];
        cnt = cnt < a.cap ? cnt : a.cap;
        const int *q = a.quads + (size_t)img * a.cap * 8;
        const unsigned full = npx > 0 ? (1u << npx) - 1u : 0u;
        for (int base = 0; base < cnt; base += VZ_QCHUNK) {
            const int m = min(VZ_QCHUNK, cnt - base);
            if (base > 0) __syncthreads();                   // the previous round has been read
            if (tid < m) {
                int p[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { p[j] = q[(size_t)(base + tid) * 8 + j]; s_pts[tid][j] = p[j]; }
                s_ext[tid][0] = min(min(p[0], p[2]), min(p[4], p[6])); s_ext[tid][1] = max(max(p[0], p[2]), max(p[4], p[6]));
                s_ext[tid][2] = min(min(p[1], p[3]), min(p[5], p[7])); s_ext[tid][3] = max(max(p[1], p[3]), max(p[5], p[7]));
            }
            __syncthreads();
            if (live) {
                for (int o = 0; o < m && m_box != full; ++o) {
                    if (y < s_ext[o][2] || y > s_ext[o][3] || x0 + npx - 1 < s_ext[o][0] || x0 > s_ext[o][1]) continue;
                    m_box |= rq_covers_run(s_pts[o], x0, npx, y, a.height);
                }
            }
        }
    }

    if (!live) return;
    const size_t off = pix * 3;
    if (want_gt) vz_emit(a.out_gt, off, px, m_gt, 0u, npx);
    if (want_seg) vz_emit(a.out_seg_map, off, px, m_seg, 0u, npx);
    if (a.out_postprocessed != nullptr) vz_emit(a.out_postprocessed, off, px, m_box, 0u, npx);
    if (want_cls) vz_emit(a.out_classification_gt, off, px, m_ok, m_bad, npx);
}

extern "C" int ubd_visualize_images(const void *images, int in_dtype, int preprocessing, int n, int height, int width, int channels,
                                    int map_h, int map_w, const int32_t *gt_labels, const int32_t *binary_map,
                                    const int32_t *quads, const int32_t *counts, int cap, const int8_t *cls_mask,
                                    uint8_t *out_gt, uint8_t *out_seg_map, uint8_t *out_postprocessed,
                                    uint8_t *out_classification_gt, void *stream)
{
    // every check comes before the first HIP call
    UBD_REQUIRE(images, "ubd_visualize_images: null images");
    UBD_REQUIRE(in_dtype == UBD_IN_U8 || in_dtype == UBD_IN_F32, "ubd_visualize_images: in_dtype must be UBD_IN_U8 or UBD_IN_F32, got %d", in_dtype);
    UBD_REQUIRE(preprocessing == UBD_PRE_NONE || preprocessing == UBD_PRE_MOBILENET, "ubd_visualize_images: unknown preprocessing %d", preprocessing);
    UBD_REQUIRE(in_dtype != UBD_IN_F32 || ((size_t)images & 3) == 0, "ubd_visualize_images: float images must be 4-byte aligned");
    UBD_REQUIRE(n >= 1, "ubd_visualize_images: n must be >= 1, got %d", n);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_visualize_images: channels must be 1 or 3, got %d", channels);
    UBD_REQUIRE(height >= 1 && width >= 1 && map_h >= 1 && map_w >= 1, "ubd_visualize_images: bad sizes %d x %d (maps %d x %d): every side must be >= 1",
                height, width, map_h, map_w);
    UBD_REQUIRE(height <= 16384 && width <= 16384, "ubd_visualize_images: image %d x %d too large: sides up to 16384", height, width);
    UBD_REQUIRE(height % map_h == 0 && width % map_w == 0 && height / map_h == width / map_w,
                "ubd_visualize_images: image %d x %d is not an integer multiple s of the maps %d x %d (the same s on both axes)", height, width, map_h, map_w);
    UBD_REQUIRE((long)n * height * width * 3 < (1L << 31), "ubd_visualize_images: n * height * width * 3 = %ld must stay below 2^31",
                (long)n * height * width * 3);
    UBD_REQUIRE(!out_gt || gt_labels, "ubd_visualize_images: out_gt given without gt_labels");
    UBD_REQUIRE(!out_seg_map || binary_map, "ubd_visualize_images: out_seg_map given without binary_map");
    UBD_REQUIRE(!out_postprocessed || (quads && counts), "ubd_visualize_images: out_postprocessed given without quads and counts");
    UBD_REQUIRE(!out_postprocessed || cap >= 1, "ubd_visualize_images: cap must be >= 1, got %d", cap);
    UBD_REQUIRE(!out_classification_gt || cls_mask, "ubd_visualize_images: out_classification_gt given without cls_mask");
    if (!out_gt && !out_seg_map && !out_postprocessed && !out_classification_gt) return 0;       // nothing asked for

    vz_args a;
    a.images = images; a.gt_labels = gt_labels; a.binary_map = binary_map; a.quads = quads; a.counts = counts; a.cls_mask = cls_mask;
    a.out_gt = out_gt; a.out_seg_map = out_seg_map; a.out_postprocessed = out_postprocessed; a.out_classification_gt = out_classification_gt;
    a.in_f32 = in_dtype == UBD_IN_F32; a.mobilenet = preprocessing == UBD_PRE_MOBILENET;
    a.height = height; a.width = width; a.channels = channels; a.map_w = map_w; a.ratio = height / map_h; a.cap = cap;
    const int runs = (width + VZ_RUN - 1) / VZ_RUN;
    a.tile_w_log2 = 0;
    while (a.tile_w_log2 < 6 && (1 << a.tile_w_log2) < runs) ++a.tile_w_log2;
    const int tile_w = 1 << a.tile_w_log2, tile_h = VZ_THREADS >> a.tile_w_log2;
    a.tiles_x = (runs + tile_w - 1) / tile_w;
    a.tiles_y = (height + tile_h - 1) / tile_h;
    const long blocks = (long)n * a.tiles_x * a.tiles_y;       // <= n * height * width: below 2^31
    hipLaunchKernelGGL(visualize_kernel, dim3((unsigned)blocks), dim3(VZ_THREADS), 0, (hipStream_t)stream, a);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
