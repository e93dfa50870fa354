// Decoding of the object patches, fifth family: Data Matrix ECC 200, the square sizes 10 x 10 to 26 x 26, out of every upright
// patch that ubd_extract_objects wrote, on the device, so that 128 bytes per object cross to the host instead of the patch.
// The rules are written out at ubd_decode_matrix_patches in include/ubd.h and restated, from the rules and not from this file,
// by the numpy oracle tests/matrix_decode_oracle.py, which this kernel matches bit for bit (tests/test_gpu_matrix_decode.py).
// The field, the placement and the codeword counts are those of the public standard (ISO/IEC 16022).  This is the one decoder
// with error correction: one Reed-Solomon block over GF(256) per symbol.
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_h, patch_w <= 128, band <= 2, window <= 64):
//   luma g <= 255; s <= 25 * 255 = 6375 (kept as uint16); d = 2 m g - lo - hi, |d| <= 12750; contrast * m <= 6375;
//   positions in 1/16 pixel: anchors 0..2048; a line's value is clamped to -32768..32767, so a product (p2 - p1) (c - c1) is
//   below 2048 * 34816 < 2^27; a sample X = (sum of four weights that add up to N^2 <= 2704, each times a corner) / N^2, the sum
//   below 2704 * 32768 < 2^27.
// The divisions of the lines and of the samples floor (dm_floor_div): a line may run to negative coordinates.
//
// Shape: one workgroup of 8 waves per patch slot; a workgroup whose slot holds no object returns after one load of counts[i].
//   1. the luma of the patch goes to LDS (one byte a pixel); meanwhile one lane builds the antilog / log tables of GF(256);
//   2. the dark map, in strips of 64 columns: a wave per row sums the (2b + 1)^2 neighbourhood into its row buffer and takes the
//      horizontal minimum and maximum of the strip's columns (two uint16 planes of 128 x 64); then a wave per row takes the
//      vertical ones down its 64 columns, and the ballot of `dark` is two words of the 2 KB bitmap (4 words a row);
//   3. column and row counts, the box, the first and last dark pixel of every row and column in the box (a thread each);
//   4. the eight anchors, a wave each: the quartile by counting ranks across the lanes; the four corners in every thread;
//   5. the 612 border modules of the nine sizes, a thread each, counted against the four turns with LDS atomics (integer
//      adds: the order does not matter); the n x n samples of the winner, a thread each, written where they lie in the symbol;
//   6. the placement walked by one lane; syndromes a lane per term; Berlekamp-Massey on one lane, its polynomials in LDS (no
//      indexed array in registers, no scratch); the Chien search and Forney's values a lane per codeword position; the
//      syndromes once more; the text and the row by one lane; the 128-byte row leaves as 32 dword stores.
// LDS: 16384 (luma) + 2 * 16384 (strip planes) + 2048 (row buffers) + 2048 (bitmap) + 3584 (the rest) = 56832 bytes.
#include "common.h"

#define DM_THREADS 512
#define DM_WAVES 8
#define DM_MIN_SIDE 32
#define DM_MAX_SIDE 128
#define DM_ROW 128
#define DM_MIN_BOX 20
#define DM_BORDERS 612                          // sum of 4 n - 4 over n = 10, 12 .. 26
#define DM_OFF_LUMA 0
#define DM_OFF_HLO 16384
#define DM_OFF_HHI 32768
#define DM_OFF_ROWBUF 49152                     // 8 waves * 128 uint16
#define DM_OFF_BITS 51200                       // 128 rows * 4 words
#define DM_OFF_CD 53248
#define DM_OFF_RD 53376
#define DM_OFF_SIDES 53504                      // left, right, top, bottom: 128 bytes each, 255 = no dark pixel
#define DM_OFF_ANCH 54016                       // 8 * (c, p)
#define DM_OFF_MISC 54080                       // 64 int32: [0..36) the finder's mismatches, [40] roots, [41] failed, [42] L, [43] degree, [44] corrected
#define DM_OFF_EXP 54336                        // antilog, 510 entries used
#define DM_OFF_LOG 54848
#define DM_OFF_CANON 55104                      // n * n bytes
#define DM_OFF_SEEN 55792                       // (n - 2)^2 bytes
#define DM_OFF_CW 56368                         // 72 codewords
#define DM_OFF_SYN 56448
#define DM_OFF_LAM 56480
#define DM_OFF_PREV 56512
#define DM_OFF_NEW 56544
#define DM_OFF_OMEGA 56576
#define DM_OFF_OUT 56608                        // the 128-byte row
#define DM_LDS_BYTES 56832                      // a multiple of 16, with 96 bytes to spare behind the row

extern __shared__ __align__(16) unsigned char dm_smem[];

// data codewords by size index (n = 10 + 2 k); check codewords
__constant__ uint8_t dm_data[9] = {3, 5, 8, 12, 18, 22, 30, 36, 44};
__constant__ uint8_t dm_check[9] = {5, 7, 10, 12, 14, 18, 20, 24, 28};

static __device__ __forceinline__ int dm_floor_div(int a, int b)       // b > 0
{
    const int q = a / b;
    return (a % b) < 0 ? q - 1 : q;
}

static __device__ __forceinline__ int dm_line(int c1, int p1, int c2, int p2, int c)
{
    const int v = p1 + dm_floor_div((p2 - p1) * (c - c1), c2 - c1);
    return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
}

struct DmCorners { int xa, ya, xb, yb, xc, yc, xd, yd; };              // TL, TR, BL, BR in 1/16 pixel

static __device__ __forceinline__ bool dm_sample(const DmCorners &K, const uint32_t *bits, int ph, int pw, int n, int r, int c)
{
    const int N = 2 * n, u = 2 * c + 1, v = 2 * r + 1;
    const int wa = (N - u) * (N - v), wb = u * (N - v), wc = (N - u) * v, wd = u * v;
    int x = dm_floor_div(wa * K.xa + wb * K.xb + wc * K.xc + wd * K.xd, N * N) >> 4;
    int y = dm_floor_div(wa * K.ya + wb * K.yb + wc * K.yc + wd * K.yd, N * N) >> 4;
    x = x < 0 ? 0 : x > pw - 1 ? pw - 1 : x;
    y = y < 0 ? 0 : y > ph - 1 ? ph - 1 : y;
    return (bits[y * 4 + (x >> 5)] >> (x & 31)) & 1u;
}

// where module (r, c) of the sampled grid lies in the symbol when the patch shows it turned by t quarter turns counter-clockwise
static __device__ __forceinline__ void dm_canonical(int n, int t, int r, int c, int &R, int &Cc)
{
    R = t == 0 ? r : t == 1 ? c : t == 2 ? n - 1 - r : n - 1 - c;
    Cc = t == 0 ? c : t == 1 ? n - 1 - r : t == 2 ? n - 1 - c : r;
}

static __device__ __forceinline__ bool dm_border_dark(int n, int r, int c)
{
    if (c == 0 || r == n - 1) return true;
    return r == 0 ? (c & 1) == 0 : (r & 1) == 1;
}

static __device__ __forceinline__ int dm_mul(const uint8_t *ex, const uint8_t *lg, int a, int b)
{
    return a && b ? ex[lg[a] + lg[b]] : 0;
}

// one bit of the placement: module (r, c) of the m x m mapping matrix with the two wrap rules; marks it seen
static __device__ __forceinline__ int dm_bit(const uint8_t *canon, uint8_t *seen, int m, int r, int c)
{
    if (r < 0) { r += m; c += 4 - (m + 4) % 8; }
    if (c < 0) { c += m; r += 4 - (m + 4) % 8; }
    seen[r * m + c] = 1;
    return canon[(r + 1) * (m + 2) + c + 1];
}

static __device__ int dm_utah(const uint8_t *canon, uint8_t *seen, int m, int r, int c)
{
    int v = dm_bit(canon, seen, m, r - 2, c - 2);
    v = 2 * v + dm_bit(canon, seen, m, r - 2, c - 1);
    v = 2 * v + dm_bit(canon, seen, m, r - 1, c - 2);
    v = 2 * v + dm_bit(canon, seen, m, r - 1, c - 1);
    v = 2 * v + dm_bit(canon, seen, m, r - 1, c);
    v = 2 * v + dm_bit(canon, seen, m, r, c - 2);
    v = 2 * v + dm_bit(canon, seen, m, r, c - 1);
    return 2 * v + dm_bit(canon, seen, m, r, c);
}

// corner case `which` (1..4): its eight modules in bit order
static __device__ int dm_corner(const uint8_t *canon, uint8_t *seen, int m, int which)
{
    int v = 0;
    for (int b = 0; b < 8; ++b) {
        int r, c;
        if (which == 1) { r = b < 3 ? m - 1 : b < 5 ? 0 : b - 4; c = b < 3 ? b : b == 3 ? m - 2 : m - 1; }
        else if (which == 2) { r = b < 3 ? m - 3 + b : b < 7 ? 0 : 1; c = b < 3 ? 0 : b < 7 ? m - 7 + b : m - 1; }
        else if (which == 3) { r = b < 3 ? m - 3 + b : b < 5 ? 0 : b - 4; c = b < 3 ? 0 : b == 3 ? m - 2 : m - 1; }
        else { r = b < 2 ? m - 1 : b < 5 ? 0 : 1; c = b == 0 ? 0 : b == 1 ? m - 1 : b < 5 ? m - 5 + b : m - 8 + b; }
        v = 2 * v + dm_bit(canon, seen, m, r, c);
    }
    return v;
}

template <int C>
__global__ __launch_bounds__(DM_THREADS) void dm_decode_kernel(const uint8_t *__restrict__ patches, const int32_t *__restrict__ counts, int cap,
                                                               int ph, int pw, int band, int window, int contrast, uint32_t *__restrict__ results)
{
    const int slot = (int)blockIdx.x;                                           // n * cap < 2^31 (checked on the host)
    const int img = slot / cap, j = slot - img * cap;
    if (j >= counts[img]) return;                                               // j < cap already
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint8_t *luma = dm_smem + DM_OFF_LUMA;
    uint16_t *hlo = (uint16_t *)(dm_smem + DM_OFF_HLO), *hhi = (uint16_t *)(dm_smem + DM_OFF_HHI);
    uint16_t *rowbuf = (uint16_t *)(dm_smem + DM_OFF_ROWBUF) + wave * DM_MAX_SIDE;
    uint32_t *bits = (uint32_t *)(dm_smem + DM_OFF_BITS);
    uint8_t *cd = dm_smem + DM_OFF_CD, *rd = dm_smem + DM_OFF_RD, *sides = dm_smem + DM_OFF_SIDES;
    int32_t *anch = (int32_t *)(dm_smem + DM_OFF_ANCH), *misc = (int32_t *)(dm_smem + DM_OFF_MISC);
    uint8_t *ex = dm_smem + DM_OFF_EXP, *lg = dm_smem + DM_OFF_LOG;
    uint8_t *canon = dm_smem + DM_OFF_CANON, *seen = dm_smem + DM_OFF_SEEN, *cw = dm_smem + DM_OFF_CW;
    uint8_t *syn = dm_smem + DM_OFF_SYN, *lam = dm_smem + DM_OFF_LAM, *prev = dm_smem + DM_OFF_PREV, *nw = dm_smem + DM_OFF_NEW;
    uint8_t *omega = dm_smem + DM_OFF_OMEGA;
    uint32_t *out_row = (uint32_t *)(dm_smem + DM_OFF_OUT);
    uint32_t *dst = results + (int64_t)slot * (DM_ROW / 4);
    const uint8_t *src = patches + (int64_t)slot * ph * pw * C;

    // 1. luma, the tables, the row of "none"
    for (int p = tid; p < ph * pw; p += DM_THREADS) {
        const uint8_t *q = src + (int64_t)p * C;
        luma[p] = (uint8_t)(C == 1 ? (int)q[0] : (19595 * (int)q[0] + 38470 * (int)q[1] + 7471 * (int)q[2] + 0x8000) >> 16);
    }
    bits[tid] = 0;                                                              // 512 words
    if (tid < 64) misc[tid] = 0;
    if (tid < DM_ROW / 4) out_row[tid] = tid < 2 ? 0u : 0xFFFFFFFFu;
    for (int p = tid; p < 576; p += DM_THREADS) seen[p] = 0;
    if (tid == DM_THREADS - 1) {
        int v = 1;
        lg[0] = 0;
        for (int k = 0; k < 255; ++k) {
            ex[k] = (uint8_t)v;
            ex[k + 255] = (uint8_t)v;
            lg[v] = (uint8_t)k;
            v <<= 1;
            if (v & 0x100) v ^= 0x12D;
        }
    }
    __syncthreads();

    // 2. the dark map
    const int m = (2 * band + 1) * (2 * band + 1), margin = contrast * m;
    for (int X0 = 0; X0 < pw; X0 += 64) {
        for (int yb = 0; yb < ph; yb += DM_WAVES) {
            const int y = yb + wave;
            const bool on = y < ph;
            if (on)
                for (int x = lane; x < pw; x += 64) {
                    int acc = 0;
                    for (int dy = -band; dy <= band; ++dy) {
                        const int yy = y + dy < 0 ? 0 : y + dy > ph - 1 ? ph - 1 : y + dy;
                        for (int dx = -band; dx <= band; ++dx) {
                            const int xx = x + dx < 0 ? 0 : x + dx > pw - 1 ? pw - 1 : x + dx;
                            acc += luma[yy * pw + xx];
                        }
                    }
                    rowbuf[x] = (uint16_t)acc;
                }
            __syncthreads();
            const int x = X0 + lane;
            if (on && x < pw) {
                const int a = x - window < 0 ? 0 : x - window, b = x + window > pw - 1 ? pw - 1 : x + window;
                int lo = rowbuf[a], hi = lo;
                for (int u = a + 1; u <= b; ++u) {
                    const int v = rowbuf[u];
                    lo = v < lo ? v : lo;
                    hi = v > hi ? v : hi;
                }
                hlo[y * 64 + lane] = (uint16_t)lo;
                hhi[y * 64 + lane] = (uint16_t)hi;
            }
            __syncthreads();
        }
        for (int yb = 0; yb < ph; yb += DM_WAVES) {
            const int y = yb + wave, x = X0 + lane;
            if (y < ph) {                                                       // uniform over the wave
                bool dark = false;
                if (x < pw) {
                    const int a = y - window < 0 ? 0 : y - window, b = y + window > ph - 1 ? ph - 1 : y + window;
                    int lo = hlo[a * 64 + lane], hi = hhi[a * 64 + lane];
                    for (int u = a + 1; u <= b; ++u) {
                        const int l = hlo[u * 64 + lane], h = hhi[u * 64 + lane];
                        lo = l < lo ? l : lo;
                        hi = h > hi ? h : hi;
                    }
                    int d = 2 * m * (int)luma[y * pw + x] - lo - hi;
                    if (hi - lo < margin && d < 1) d = 1;
                    dark = d < -margin;
                }
                const unsigned long long mask = __ballot(dark);
                if (lane == 0) {
                    bits[y * 4 + (X0 >> 5)] = (uint32_t)mask;
                    bits[y * 4 + (X0 >> 5) + 1] = (uint32_t)(mask >> 32);
                }
            }
        }
        __syncthreads();                                                        // the next strip overwrites the planes
    }

    // 3. counts, box, sides
    if (tid < 128) {
        int n = 0;
        if (tid < pw)
            for (int y = 0; y < ph; ++y) n += (bits[y * 4 + (tid >> 5)] >> (tid & 31)) & 1u;
        cd[tid] = (uint8_t)n;
    } else if (tid < 256) {
        const int y = tid - 128;
        rd[y] = (uint8_t)(y < ph ? __popc(bits[y * 4]) + __popc(bits[y * 4 + 1]) + __popc(bits[y * 4 + 2]) + __popc(bits[y * 4 + 3]) : 0);
    }
    __syncthreads();
    int x0 = -1, x1 = -1, y0 = -1, y1 = -1;
    {
        int mx = 0, my = 0;
        for (int k = 0; k < 128; ++k) {
            mx = cd[k] > mx ? cd[k] : mx;
            my = rd[k] > my ? rd[k] : my;
        }
        const int tx = mx / 4 < 1 ? 1 : mx / 4, ty = my / 4 < 1 ? 1 : my / 4;
        for (int k = 0; k < 128; ++k) {
            if (cd[k] >= tx) { x0 = x0 < 0 ? k : x0; x1 = k; }
            if (rd[k] >= ty) { y0 = y0 < 0 ? k : y0; y1 = k; }
        }
    }
    if (x0 < 0 || y0 < 0 || x1 - x0 + 1 < DM_MIN_BOX || y1 - y0 + 1 < DM_MIN_BOX) {    // uniform: every thread read the same counts
        if (tid < DM_ROW / 4) dst[tid] = out_row[tid];
        return;
    }
    if (tid < 128) {                                                            // left, right of row tid
        int first = 255, last = 255;
        if (tid >= y0 && tid <= y1)
            for (int w = 0; w < 4; ++w) {
                const int lo = x0 - 32 * w < 0 ? 0 : x0 - 32 * w, hi = x1 - 32 * w > 31 ? 31 : x1 - 32 * w;
                if (lo > hi) continue;
                const uint32_t word = bits[tid * 4 + w] & (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
                if (word) {
                    if (first == 255) first = 32 * w + __ffs((int)word) - 1;
                    last = 32 * w + 32 - __clz((int)word);                      // the last dark x plus 1
                }
            }
        sides[tid] = (uint8_t)first;
        sides[128 + tid] = (uint8_t)last;
    } else if (tid < 256) {                                                     // top, bottom of column tid - 128
        const int x = tid - 128;
        int first = 255, last = 255;
        if (x >= x0 && x <= x1)
            for (int y = y0; y <= y1; ++y)
                if ((bits[y * 4 + (x >> 5)] >> (x & 31)) & 1u) {
                    if (first == 255) first = y;
                    last = y + 1;
                }
        sides[256 + x] = (uint8_t)first;
        sides[384 + x] = (uint8_t)last;
    }
    __syncthreads();

    // 4. the anchors: wave = 2 * side + segment; sides: left, right, top, bottom
    {
        const int side = wave >> 1, seg = wave & 1;
        const int a0 = side < 2 ? y0 : x0, a1 = side < 2 ? y1 : x1, L = a1 - a0 + 1;
        const int s0 = seg ? a1 - L / 2 + 1 : a0 + L / 16, s1 = seg ? a1 - L / 16 : a0 + L / 2 - 1;     // at most 56 values
        const int at = s0 + lane;
        const int v = at <= s1 ? (int)sides[side * 128 + at] : 255;
        const bool valid = v != 255;
        const int count = __popcll(__ballot(valid));
        const int key = !valid ? 1 << 20 : (side & 1) ? -v : v;                 // right and bottom: the k-th largest
        int rank = 0;
        for (int l = 0; l < 64; ++l) {
            const int other = __shfl(key, l);
            rank += other < key || (other == key && l < lane);
        }
        if (lane == 0) anch[2 * wave] = -1;
        if (count >= 4 && valid && rank == count / 4) {                         // lane 0's store above comes first in program order
            anch[2 * wave] = 8 * (s0 + s1 + 1);
            anch[2 * wave + 1] = 16 * v;
        }
    }
    __syncthreads();
    bool fine = true;
    for (int k = 0; k < 8; ++k) fine = fine && anch[2 * k] >= 0;
    if (!fine) {
        if (tid < DM_ROW / 4) dst[tid] = out_row[tid];
        return;
    }
    DmCorners K;
    {
        const int xm = 8 * (x0 + x1 + 1);
#define DM_HOR(s, x) dm_line(anch[4 * (s)], anch[4 * (s) + 1], anch[4 * (s) + 2], anch[4 * (s) + 3], x)
#define DM_CORNER(hs, vs, X, Y)                                                          \
    {                                                                                    \
        int yy = DM_HOR(hs, xm), xx = 0;                                                 \
        for (int it = 0; it < 3; ++it) { xx = DM_HOR(vs, yy); yy = DM_HOR(hs, xx); }     \
        X = xx; Y = yy;                                                                  \
    }
        DM_CORNER(2, 0, K.xa, K.ya)
        DM_CORNER(2, 1, K.xb, K.yb)
        DM_CORNER(3, 0, K.xc, K.yc)
        DM_CORNER(3, 1, K.xd, K.yd)
#undef DM_CORNER
#undef DM_HOR
    }

    // 5. the finder: the border modules of the nine sizes against the four turns
    for (int item = tid; item < DM_BORDERS; item += DM_THREADS) {
        int si = 0;
        while (si < 8 && item >= 36 * (si + 1) + 4 * (si + 1) * si) ++si;       // the borders of the sizes before si + 1
        const int n = 10 + 2 * si, b = item - (36 * si + 4 * si * (si - 1));
        int r, c;
        if (b < n) { r = 0; c = b; }
        else if (b < 2 * n - 1) { r = b - n + 1; c = n - 1; }
        else if (b < 3 * n - 2) { r = n - 1; c = b - (2 * n - 1); }
        else { r = b - (3 * n - 2) + 1; c = 0; }
        const bool g = dm_sample(K, bits, ph, pw, n, r, c);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int R, Cc;
            dm_canonical(n, t, r, c, R, Cc);
            if (g != dm_border_dark(n, R, Cc)) atomicAdd(&misc[si * 4 + t], 1);
        }
    }
    __syncthreads();
    int best = 1 << 20, best_at = 0, ties = 0;
    for (int k = 0; k < 36; ++k) {
        const int v = misc[k];
        if (v < best) { best = v; best_at = k; ties = 1; }
        else if (v == best) ++ties;
    }
    const int si = best_at >> 2, turns = best_at & 3, n = 10 + 2 * si;
    if (8 * best > 4 * n - 4 || ties != 1) {
        if (tid < DM_ROW / 4) dst[tid] = out_row[tid];
        return;
    }
    for (int item = tid; item < n * n; item += DM_THREADS) {
        const int r = item / n, c = item - r * n;
        int R, Cc;
        dm_canonical(n, turns, r, c, R, Cc);
        canon[R * n + Cc] = (uint8_t)dm_sample(K, bits, ph, pw, n, r, c);
    }
    __syncthreads();

    // 6. codewords, Reed-Solomon, text
    const int nd = dm_data[si], e = dm_check[si], total = nd + e, mm = n - 2;
    if (tid == 0) {                                                             // the placement of ISO/IEC 16022 Annex F, walked
        int k = 0, r = 4, c = 0;
        do {
            if (r == mm && c == 0) cw[k++] = (uint8_t)dm_corner(canon, seen, mm, 1);
            if (r == mm - 2 && c == 0 && mm % 4 != 0) cw[k++] = (uint8_t)dm_corner(canon, seen, mm, 2);
            if (r == mm - 2 && c == 0 && mm % 8 == 4) cw[k++] = (uint8_t)dm_corner(canon, seen, mm, 3);
            if (r == mm + 4 && c == 2 && mm % 8 == 0) cw[k++] = (uint8_t)dm_corner(canon, seen, mm, 4);
            do {
                if (r < mm && c >= 0 && !seen[r * mm + c] && k < total) cw[k++] = (uint8_t)dm_utah(canon, seen, mm, r, c);
                r -= 2; c += 2;
            } while (r >= 0 && c < mm);
            r += 1; c += 3;
            do {
                if (r >= 0 && c < mm && !seen[r * mm + c] && k < total) cw[k++] = (uint8_t)dm_utah(canon, seen, mm, r, c);
                r += 2; c -= 2;
            } while (r < mm && c >= 0);
            r += 3; c += 1;
        } while (r < mm || c < mm);
    }
    if (tid < 32) { lam[tid] = tid == 0; prev[tid] = tid == 0; omega[tid] = 0; }
    __syncthreads();
    if (tid < e) {                                                              // S_j = r(a^j), j = tid + 1, by Horner's rule
        int v = 0;
        for (int i = 0; i < total; ++i) v = (v ? ex[lg[v] + tid + 1] : 0) ^ cw[i];
        syn[tid] = (uint8_t)v;
    }
    __syncthreads();
    bool clean = true;
    for (int i = 0; i < e; ++i) clean = clean && syn[i] == 0;
    if (!clean) {                                                               // uniform
        if (tid == 0) {                                                         // Berlekamp-Massey
            int L = 0, shift = 1, b = 1;
            for (int k = 0; k < e; ++k) {
                int delta = syn[k];
                for (int i = 1; i <= L; ++i) delta ^= dm_mul(ex, lg, lam[i], syn[k - i]);
                if (delta == 0) { ++shift; continue; }
                const int scale = dm_mul(ex, lg, delta, ex[255 - lg[b]]);
                for (int i = 0; i < 32; ++i) nw[i] = lam[i] ^ (uint8_t)(i >= shift ? dm_mul(ex, lg, scale, prev[i - shift]) : 0);
                if (2 * L <= k) {
                    for (int i = 0; i < 32; ++i) prev[i] = lam[i];
                    L = k + 1 - L; b = delta; shift = 1;
                } else {
                    ++shift;
                }
                for (int i = 0; i < 32; ++i) lam[i] = nw[i];
            }
            int degree = 0;
            for (int i = 0; i < 32; ++i) degree = lam[i] ? i : degree;
            misc[42] = L;
            misc[43] = degree;
        }
        __syncthreads();
        const int L = misc[42], degree = misc[43];
        if (L > e / 2 || degree != L) {
            if (tid < DM_ROW / 4) dst[tid] = out_row[tid];
            return;
        }
        if (tid < e) {                                                          // omega = S(x) lambda(x) mod x^e
            int v = 0;
            for (int q = 0; q <= (tid < degree ? tid : degree); ++q) v ^= dm_mul(ex, lg, lam[q], syn[tid - q]);
            omega[tid] = (uint8_t)v;
        }
        bool root = false;
        int xinv = 1;
        if (tid < total) {                                                      // the codeword at the power tid of x
            xinv = ex[(255 - tid) % 255];
            int v = 0;
            for (int i = degree; i >= 0; --i) v = dm_mul(ex, lg, v, xinv) ^ lam[i];
            root = v == 0;
            if (root) atomicAdd(&misc[40], 1);
        }
        __syncthreads();
        if (root) {                                                             // Forney: omega(1 / X) / lambda'(1 / X)
            int deriv = 0, om = 0;
            for (int i = 1; i <= degree; i += 2) deriv ^= dm_mul(ex, lg, lam[i], ex[(lg[xinv] * (i - 1)) % 255]);
            for (int i = e - 1; i >= 0; --i) om = dm_mul(ex, lg, om, xinv) ^ omega[i];
            if (deriv == 0) misc[41] = 1;
            else cw[total - 1 - tid] ^= (uint8_t)dm_mul(ex, lg, om, ex[255 - lg[deriv]]);
        }
        __syncthreads();
        if (tid < e) {                                                          // the corrected word's syndromes must vanish
            int v = 0;
            for (int i = 0; i < total; ++i) v = (v ? ex[lg[v] + tid + 1] : 0) ^ cw[i];
            if (v) misc[41] = 1;
        }
        __syncthreads();
        if (misc[40] != degree || misc[41]) {
            if (tid < DM_ROW / 4) dst[tid] = out_row[tid];
            return;
        }
        if (tid == 0) misc[44] = degree;                                        // ordered before its read by the barrier below
    }
    __syncthreads();
    if (tid == 0) {                                                             // the text and the row
        uint8_t *row = (uint8_t *)out_row;
        int t = 0, flags = 0, k = 0, u = 0;
        for (; k < nd; ++k) {
            const int v = cw[k];
            if (v >= 1 && v <= 128) row[8 + t++] = (uint8_t)(v - 1);
            else if (v >= 130 && v <= 229) { row[8 + t++] = (uint8_t)(48 + (v - 130) / 10); row[8 + t++] = (uint8_t)(48 + (v - 130) % 10); }
            else if (v == 235 && k + 1 < nd && cw[k + 1] >= 1 && cw[k + 1] <= 128) row[8 + t++] = (uint8_t)(cw[++k] + 127);
            else if (v == 129) break;
            else if (v == 232 && k == 0) flags |= 1;
            else if (v == 232) row[8 + t++] = 0x1D;
            else {
                flags |= 2;
                for (; k < nd; ++k) row[8 + t + u++] = cw[k];                   // t + u <= 2 * 44: within the row
                break;
            }
        }
        row[0] = 68; row[1] = (uint8_t)n; row[2] = (uint8_t)turns; row[3] = (uint8_t)t;
        row[4] = (uint8_t)flags; row[5] = (uint8_t)misc[44]; row[6] = (uint8_t)best; row[7] = (uint8_t)u;
    }
    __syncthreads();
    if (tid < DM_ROW / 4) dst[tid] = out_row[tid];
}

extern "C" int ubd_decode_matrix_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                                         const ubd_decode_params *params, uint8_t *results, void *launch_stream)
{
    const char *who = "ubd_decode_matrix_patches";
    UBD_REQUIRE(patches, "%s: patches is null", who);
    UBD_REQUIRE(counts, "%s: counts is null", who);
    UBD_REQUIRE(params, "%s: params is null", who);
    UBD_REQUIRE(results, "%s: results is null", who);
    UBD_REQUIRE(((uintptr_t)results & 3) == 0, "%s: results must be aligned to 4 bytes", who);
    UBD_REQUIRE(n >= 1, "%s: n must be >= 1, got %d", who, n);
    UBD_REQUIRE(cap >= 1, "%s: cap must be >= 1, got %d", who, cap);
    UBD_REQUIRE(patch_h >= DM_MIN_SIDE && patch_h <= DM_MAX_SIDE, "%s: patch_h must be %d..%d, got %d", who, DM_MIN_SIDE, DM_MAX_SIDE, patch_h);
    UBD_REQUIRE(patch_w >= DM_MIN_SIDE && patch_w <= DM_MAX_SIDE, "%s: patch_w must be %d..%d, got %d", who, DM_MIN_SIDE, DM_MAX_SIDE, patch_w);
    UBD_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, channels);
    const ubd_decode_params P = *params;
    UBD_REQUIRE(P.symbologies == 32768,
                "%s: symbologies must be 32768 (bit 15, Data Matrix; bit 14 is unassigned, the lower bits are the other four entry points'), got %d",
                who, P.symbologies);
    UBD_REQUIRE(P.scan_rows >= 1 && P.scan_rows <= 32, "%s: scan_rows must be 1..32, got %d", who, P.scan_rows);
    UBD_REQUIRE(P.band >= 0 && P.band <= 2, "%s: band must be 0..2, got %d", who, P.band);
    UBD_REQUIRE(P.window >= 1 && P.window <= 64, "%s: window must be 1..64, got %d", who, P.window);
    UBD_REQUIRE(P.contrast >= 0 && P.contrast <= 255, "%s: contrast must be 0..255, got %d", who, P.contrast);
    UBD_REQUIRE(P.quiet >= 0 && P.quiet <= 16, "%s: quiet must be 0..16, got %d", who, P.quiet);
    UBD_REQUIRE(P.min_votes >= 1 && P.min_votes <= 2 * P.scan_rows, "%s: min_votes must be 1..2 * scan_rows = %d, got %d", who, 2 * P.scan_rows,
                P.min_votes);
    UBD_REQUIRE((int64_t)n * cap < ((int64_t)1 << 31), "%s: n * cap = %d * %d is not below 2^31", who, n, cap);
    const dim3 grid((unsigned)((int64_t)n * cap)), block(DM_THREADS);
    if (channels == 3)
        hipLaunchKernelGGL((dm_decode_kernel<3>), grid, block, DM_LDS_BYTES, (hipStream_t)launch_stream, patches, counts, cap, patch_h, patch_w,
                           P.band, P.window, P.contrast, (uint32_t *)results);
    else
        hipLaunchKernelGGL((dm_decode_kernel<1>), grid, block, DM_LDS_BYTES, (hipStream_t)launch_stream, patches, counts, cap, patch_h, patch_w,
                           P.band, P.window, P.contrast, (uint32_t *)results);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
