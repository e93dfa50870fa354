// The part of the patch decoders that does not know a symbology: the profile of a scan line, its local threshold and its
// sub-pixel edges, as the rules at ubd_decode_patches in include/ubd.h define them, and the edge list as one reading direction
// sees it.  decode.hip (EAN-13 / UPC-A / EAN-8) and decode_text.hip (Code 128) include it; both kernels have the same shape,
// one workgroup of DC_WAVES waves per patch slot and one wave per scan line.
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_w <= 1024, band <= 8, window <= 64):
//   profile p <= 17 rows * 255 = 4335; d = 2p - lo - hi, |d| <= 8670 (kept as int16); contrast * m <= 255 * 17;
//   edge e = 256 x + 256 |d| / (|d| + |d'|) <= 256 * 1023 = 261888 < 2^18, so every run and every sum of runs is < 2^18.
// The one division (the edge position) has a non-negative dividend, so C's truncation is the floor of the rules.
#pragma once
#include "common.h"

#define DC_WAVES 8
#define DC_THREADS (DC_WAVES * 64)
#define DC_MAX_W 1024
#define DC_MIN_W 32
#define DC_MAX_H 1024
#define DC_MAX_ROWS 32

struct DcLine {                 // the edge list of one scan line as one reading direction sees it
    const int32_t *e;           // positions in 1/256 pixel, left to right
    int n;                      // number of edges
    int flip;                   // 256 * (patch_w - 1)
    int l2d0;                   // 1: the first edge, left to right, goes from light to dark (polarities alternate)
    bool rev;                   // the mirrored list e'_j = flip - e_(n-1-j), polarities swapped
};

static __device__ __forceinline__ int dc_edge(const DcLine &L, int j) { return L.rev ? L.flip - L.e[L.n - 1 - j] : L.e[j]; }

static __device__ __forceinline__ bool dc_light_to_dark(const DcLine &L, int j)
{
    return L.rev ? !((L.l2d0 ^ (L.n - 1 - j)) & 1) : ((L.l2d0 ^ j) & 1);
}

// bytes of LDS the waves' lines take behind a kernel's own tables: per wave patch_w int32 (the profile, over which the edge
// list is later written: p is dead by then, and there are at most patch_w - 1 edges) and patch_w int16 (d)
static inline size_t dc_lines_bytes(int patch_w) { return (size_t)DC_WAVES * ((patch_w + 1) & ~1) * 6; }       // <= 49152

// The three stages of scan line k of S for the calling wave: profile, threshold, edges.  Called by every wave of the workgroup
// (the two barriers between the stages are uniform; `on` is false for a wave beyond the last line, which idles between them).
// lines: the LDS behind the kernel's tables (dc_lines_bytes).  Leaves the edges in `pe`, their number in n_edges and the
// polarity of the first in l2d0; the caller puts a barrier before it reads them.  The sliding minimum and maximum are the plain
// loop over the 2R + 1 neighbours; the edges are compacted in order, 64 pixels a step, with a ballot and the popcount of the
// lanes below.
template <int C>
static __device__ __forceinline__ void dc_scan_line(const uint8_t *__restrict__ src, int ph, int pw, int k, int S, bool on, int wave, int lane,
                                                    const ubd_decode_params &P, unsigned char *lines, int32_t *&pe, int &n_edges, int &l2d0)
{
    const int pwp = (pw + 1) & ~1;                                              // int16 rows end on a dword boundary
    pe = (int32_t *)(lines + (size_t)wave * pwp * 6);                           // pw int32: the profile, then the edges (at most pw - 1)
    int16_t *dd = (int16_t *)(pe + pwp);                                        // pw int16: d
    const unsigned long long below = (1ull << lane) - 1ull;
    int m = 1;
    if (on) {                                                                   // the profile of scan line k
        const int r = ((2 * k + 1) * ph) / (2 * S);
        const int r0 = r - P.band < 0 ? 0 : r - P.band, r1 = r + P.band > ph - 1 ? ph - 1 : r + P.band;
        m = r1 - r0 + 1;
        for (int x = lane; x < pw; x += 64) {
            int acc = 0;
            for (int y = r0; y <= r1; ++y) {
                const uint8_t *q = src + ((int64_t)y * pw + x) * C;
                acc += C == 1 ? (int)q[0] : (19595 * (int)q[0] + 38470 * (int)q[1] + 7471 * (int)q[2] + 0x8000) >> 16;
            }
            pe[x] = acc;
        }
    }
    __syncthreads();
    if (on) {                                                                   // the local threshold
        const int flat = P.contrast * m;
        for (int x = lane; x < pw; x += 64) {
            const int x0 = x - P.window < 0 ? 0 : x - P.window, x1 = x + P.window > pw - 1 ? pw - 1 : x + P.window;
            int lo = pe[x0], hi = lo;
            for (int u = x0 + 1; u <= x1; ++u) {
                const int v = pe[u];
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            int d = 2 * pe[x] - lo - hi;
            if (hi - lo < flat && d < 1) d = 1;
            dd[x] = (int16_t)d;
        }
    }
    __syncthreads();
    n_edges = 0;
    l2d0 = 0;
    if (on) {                                                                   // the edges, in order; they overwrite the profile
        for (int xb = 0; xb < pw - 1; xb += 64) {
            const int x = xb + lane;
            bool is = false, l2d = false;
            int pos = 0;
            if (x < pw - 1) {
                const int a = dd[x], b = dd[x + 1];
                is = (a < 0) != (b < 0);
                if (is) {
                    const int aa = a < 0 ? -a : a, bb = b < 0 ? -b : b;         // aa + bb >= 1: one of them is negative
                    pos = 256 * x + (256 * aa) / (aa + bb);
                    l2d = b < 0;
                }
            }
            const unsigned long long mask = __ballot(is), dark = __ballot(l2d);
            if (is) pe[n_edges + __popcll(mask & below)] = pos;                 // n_edges + 63 <= pw - 2: one edge per pixel pair at most
            if (n_edges == 0 && mask) l2d0 = (int)((dark >> (__ffsll((long long)mask) - 1)) & 1ull);
            n_edges += __popcll(mask);
        }
    }
}
