// Decoding of the object patches, fourth family: the postal height-modulated codes POSTNET, PLANET, RM4SCC and KIX, out of every
// upright patch that ubd_extract_objects wrote, on the device, so that 128 bytes per object cross to the host instead of the
// patch.  The rules are written out at ubd_decode_postal_patches in include/ubd.h and restated, from the rules and not from this
// file, by the numpy oracle tests/postal_decode_oracle.py, which this kernel matches bit for bit (tests/test_gpu_postal_decode.py).
// The bar tables are those of the public descriptions of the codes (USPS Publication 25; Royal Mail's 4-state customer code).
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_w, patch_h <= 1024, window <= 64, quiet <= 16):
//   luma g <= 255; thr = Lmin + Lmax <= 510; d = 2 g - thr, |d| <= 510; 256 |d| <= 130560;
//   bar positions s, t <= 256 * 1023 = 261888 < 2^18 (an edge lies between two pixels of the patch); s + t + 256 < 2^19;
//   pitch p < 2^18: 3 p, 4 p, 5 p, 4 (t - s) < 2^21; 2 p / 256 < 2^11;
//   rows: top, bot, T, Bm, q, r in 0..1023; a = -top in -1023..0, c = bot; lo + hi, 2 w in -2046..2046; 5 (hi - lo) <= 5115; Hs <= 1024;
//   quiet zones: B <= 122, so (2 B - 1) q <= 243 * 2^18 < 2^26; QZ * St <= 16 * 2^18 = 2^22; the divisor (2 B - 1) * 256 <= 62208;
//   checks: at most 14 digits, sum <= 126; at most 29 values of 1..6, sums <= 174.
// The divisions (an edge position, q, the quiet pixels) have non-negative dividends, so C's truncation is the floor of the rules.
//
// Shape: one workgroup of DC_WAVES waves per patch slot, one wave per scan line, DC_WAVES lines per round, the front end of a
// round that of the other families (dc_scan_line of decode_scan.h).  The round loop is this file's own, because a candidate
// here is not a function of the edge list: one lane per start edge walks its chain of bars on the patch, 64 starts a step in
// rising order.  The walk does not depend on the symbology beyond G, the number of bars the tracking row remembers, so a
// direction of a line is walked once per G and both symbologies of that G are judged from it.  The first walk keeps no bars:
// it gives the number of bars, the chain's extent, its tallest bar and the quiet zones.  Few lanes pass that (the bar count
// must fit a symbology that is asked for); they go in rising order, one lane at a time: the lane walks once more, now
// writing top and bot of every bar into the wave's 512 bytes of LDS, and judges the bars from there, so no lane holds an
// array and nothing spills.  A valid reading goes straight into the vote slot (line, direction, symbology): 32 bytes,
// [0] T, [1] the symbology's code, [2..] the characters, zeroes behind.  The tally compares whole slots; thread 0 builds the
// winner's 128-byte row in LDS, which leaves as 32 dword stores.  Luma is read straight from the patch (L1 / L2).
// LDS: 8192 (votes) + 1024 (tally) + 4096 (bars) + 128 (row) + at most 49152 (lines) = 62592 bytes.
#include "decode_scan.h"

#define PD_SYMS 4                               // POSTNET, PLANET, RM4SCC, KIX: the bits 10..13, the symbology index is bit - 10
#define PD_MAX_VOTES (2 * PD_SYMS * DC_MAX_ROWS)
#define PD_SLOT 32                              // bytes of a vote slot
#define PD_MAX_BARS 122
#define PD_ROW 128                              // bytes of a result row
#define PD_WAVE_BARS 512                        // bytes of a wave's bars: (top, bot) as int16, 123 at most
#define PD_OFF_TALLY (PD_MAX_VOTES * PD_SLOT)
#define PD_OFF_BARS (PD_OFF_TALLY + PD_MAX_VOTES * 4)
#define PD_OFF_ROW (PD_OFF_BARS + DC_WAVES * PD_WAVE_BARS)
#define PD_TABLE_BYTES (PD_OFF_ROW + PD_ROW)    // 13440, a multiple of 16

__constant__ uint8_t pd_codes[PD_SYMS] = {80, 76, 82, 75};
// the digit of a POSTNET word of five bars (the first bar the most significant bit, 1 = long), -1: no digit
__constant__ int8_t pd_digit[32] = {-1, -1, -1, 1, -1, 2, 3, -1, -1, 4, 5, -1, 6, -1, -1, -1, -1, 7, 8, -1, 9, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1};
// the index of a 4-state word of four bars: 0011 0101 0110 1001 1010 1100 -> 0..5
__constant__ int8_t pd_four[16] = {-1, -1, -1, 0, -1, 1, 2, -1, -1, 3, 4, -1, 5, -1, -1, -1};

// the luma of one reading direction: direction 1 reads the half-turned patch
template <int C>
struct PdImage {
    const uint8_t *src;
    int h, w;
    bool turned;
    __device__ __forceinline__ int g(int y, int x) const
    {
        if (turned) { y = h - 1 - y; x = w - 1 - x; }
        const uint8_t *q = src + ((int64_t)y * w + x) * C;
        return C == 1 ? (int)q[0] : (19595 * (int)q[0] + 38470 * (int)q[1] + 7471 * (int)q[2] + 0x8000) >> 16;
    }
};

struct PdChain { int bars, s_first, t_last, row, thr, tallest; };   // row, thr: what the last bar left

// The chain of bars from the bar [s, t] on row r; false for a chain of more than PD_MAX_BARS bars.  STORE: top and bot of bar b
// go to store[2 b], store[2 b + 1].
template <int C, bool STORE>
static __device__ bool pd_walk(const PdImage<C> &I, int r, int s, int t, int G, int window, int contrast, int16_t *store, PdChain &ch)
{
    int tp[5], bt[5];                           // the last five bars, the newest first (static indices: registers)
#pragma unroll
    for (int k = 0; k < 5; ++k) { tp[k] = 0; bt[k] = I.h; }
    int n = 0, s_prev = 0, p = 0, p_prev = 0;
    ch.s_first = s; ch.t_last = t; ch.row = r; ch.thr = 0; ch.tallest = 0;
    for (;;) {
        const int xc = (s + t + 256) >> 9;
        const int x0 = xc - window < 0 ? 0 : xc - window, x1 = xc + window > I.w - 1 ? I.w - 1 : xc + window;
        int lmin = I.g(r, x0), lmax = lmin;
        for (int u = x0 + 1; u <= x1; ++u) {
            const int v = I.g(r, u);
            lmin = v < lmin ? v : lmin;
            lmax = v > lmax ? v : lmax;
        }
        const int thr = lmin + lmax;
        if (lmax - lmin < contrast || 2 * I.g(r, xc) >= thr) break;
        if (n >= 1) {
            p = s - s_prev;
            if (4 * (t - s) > 3 * p) break;
            if (n >= 2 && (3 * p_prev > 4 * p || 4 * p > 5 * p_prev)) break;
        }
        int top = r, bot = r;
        while (top > 0 && 2 * I.g(top - 1, xc) < thr) --top;
        while (bot < I.h - 1 && 2 * I.g(bot + 1, xc) < thr) ++bot;
#pragma unroll
        for (int k = 4; k >= 1; --k) { tp[k] = tp[k - 1]; bt[k] = bt[k - 1]; }
        tp[0] = top; bt[0] = bot;
        if (n + 1 >= G) {                       // the tracking row
            int hi_top = tp[0], lo_bot = bt[0];
#pragma unroll
            for (int k = 1; k < 5; ++k)
                if (k < G) {
                    hi_top = tp[k] > hi_top ? tp[k] : hi_top;
                    lo_bot = bt[k] < lo_bot ? bt[k] : lo_bot;
                }
            if (lo_bot < hi_top) break;
            const int q = (lo_bot - hi_top) >> 2;
            r = r < hi_top + q ? hi_top + q : r;
            r = r > lo_bot - q ? lo_bot - q : r;
        }
        if (STORE) { store[2 * n] = (int16_t)top; store[2 * n + 1] = (int16_t)bot; }   // n <= 122: bytes 0..491
        ++n;
        ch.t_last = t; ch.row = r; ch.thr = thr;
        ch.tallest = bot - top + 1 > ch.tallest ? bot - top + 1 : ch.tallest;
        if (n > PD_MAX_BARS) return false;
        s_prev = s; p_prev = p;
        // the next bar, on the (moved) row with this bar's thr
        int x = (t >> 8) + 1;
        int end = x + (n == 1 ? window : (2 * p) >> 8);
        end = end > I.w - 1 ? I.w - 1 : end;
        if (x >= end) break;
        int d0 = 2 * I.g(r, x) - thr, d1 = 0;
        bool found = false;
        for (; x < end; ++x) {
            d1 = 2 * I.g(r, x + 1) - thr;
            if (d0 >= 0 && d1 < 0) { found = true; break; }
            d0 = d1;
        }
        if (!found) break;
        s = 256 * x + (256 * d0) / (d0 - d1);
        ++x;                                    // d1 is d(x) of the new x
        end = x + window > I.w - 1 ? I.w - 1 : x + window;
        found = false;
        d0 = d1;
        for (; x < end; ++x) {
            d1 = 2 * I.g(r, x + 1) - thr;
            if (d0 < 0 && d1 >= 0) { found = true; break; }
            d0 = d1;
        }
        if (!found) break;
        t = 256 * x + (256 * -d0) / (d1 - d0);
    }
    ch.bars = n;
    return true;
}

// the number of characters of a symbol of `sym` with `bars` bars, 0 where that is no length of the symbology
static __device__ __forceinline__ int pd_chars(int sym, int bars)
{
    if (sym == 0) return bars == 32 || bars == 37 || bars == 52 || bars == 62 ? (bars - 2) / 5 : 0;
    if (sym == 1) return bars == 62 || bars == 72 ? (bars - 2) / 5 : 0;
    if (sym == 2) return bars % 4 == 2 && bars >= 10 ? (bars - 2) / 4 : 0;     // bars <= 122: at most 30
    return bars % 4 == 0 && bars >= 16 && bars <= 120 ? bars / 4 : 0;
}

// The quiet zones of the chain that starts at edge i of L.
template <int C>
static __device__ bool pd_quiet(const PdImage<C> &I, const DcLine &L, int i, const PdChain &ch, int quiet)
{
    const int st = ch.t_last - ch.s_first, k = 2 * ch.bars - 1;
    if (i >= 1 && k * (dc_edge(L, i) - dc_edge(L, i - 1)) < quiet * st) return false;
    const int x0 = (ch.t_last >> 8) + 1;
    int x1 = x0 + (quiet * st + k * 256 - 1) / (k * 256);
    x1 = x1 > I.w ? I.w : x1;
    for (int x = x0; x < x1; ++x)
        if (2 * I.g(ch.row, x) < ch.thr) return false;
    return true;
}

// The stored bars as one symbol of `sym` (n characters): its characters go to out (n bytes); false where it is none, with
// out left in any state.
static __device__ bool pd_judge(const int16_t *store, int bars, int tallest, int sym, int n, uint8_t *out)
{
    const int G = sym < 2 ? 5 : 4;
    const bool framed = sym != 3;
    int sum = 0, rows = 0, cols = 0;
    for (int k = 0; k < n; ++k) {
        const int base = framed ? 1 + G * k : G * k;
        const int first = framed && k == 0 ? 0 : base, last = framed && k == n - 1 ? bars - 1 : base + G - 1;
        int lo_a = -store[2 * first], hi_a = lo_a, lo_c = store[2 * first + 1], hi_c = lo_c;
        for (int b = first + 1; b <= last; ++b) {
            const int a = -store[2 * b], c = store[2 * b + 1];
            lo_a = a < lo_a ? a : lo_a; hi_a = a > hi_a ? a : hi_a;
            lo_c = c < lo_c ? c : lo_c; hi_c = c > hi_c ? c : hi_c;
        }
        const bool any_a = 5 * (hi_a - lo_a) >= tallest, any_c = 5 * (hi_c - lo_c) >= tallest;
        int wa = 0, wc = 0;
        for (int b = first; b <= last; ++b) {
            const bool la = any_a && 2 * -store[2 * b] > lo_a + hi_a, lc = any_c && 2 * store[2 * b + 1] > lo_c + hi_c;
            if (b < base) {                     // the opening frame bar: long in a; in c it is not
                if (!la || lc) return false;
            } else if (b >= base + G) {         // the closing frame bar: long in a; in c only that of an RM4SCC
                if (!la || lc != (sym == 2)) return false;
            } else {
                wa = wa << 1 | (int)la;
                wc = wc << 1 | (int)lc;
            }
        }
        if (sym < 2) {
            if (wc) return false;
            const int d = pd_digit[sym == 1 ? wa ^ 31 : wa];
            if (d < 0) return false;
            sum += d;
            out[k] = (uint8_t)(48 + d);
        } else {
            const int ia = pd_four[wa], ic = pd_four[wc];
            if ((ia | ic) < 0) return false;
            const int v = 6 * ia + ic;
            if (sym == 2 && k == n - 1) {
                if (v != 6 * ((rows % 6 + 5) % 6) + (cols % 6 + 5) % 6) return false;
            }
            rows += ia + 1;
            cols += ic + 1;
            out[k] = (uint8_t)(v < 10 ? 48 + v : 55 + v);
        }
    }
    return sym >= 2 || sum % 10 == 0;
}

// What dc_winner needs of a family, and the vote table.
struct PdPostal {
    static __device__ __forceinline__ uint32_t *votes(int u) { return (uint32_t *)dc_smem + u * (PD_SLOT / 4); }
    static __device__ __forceinline__ bool empty(int u) { return (votes(u)[0] & 0xFFu) == 0; }
    static __device__ __forceinline__ bool same(int u, int v)
    {
        const uint32_t *a = votes(u), *b = votes(v);
        bool same = true;
#pragma unroll
        for (int q = 0; q < PD_SLOT / 4; ++q) same = same && a[q] == b[q];
        return same;
    }
    static int check_results(const char *who, const void *results)
    {
        UBD_REQUIRE(((uintptr_t)results & 3) == 0, "%s: results must be aligned to 4 bytes", who);
        return 0;
    }
    static int check_symbologies(const char *who, int symbologies)
    {
        UBD_REQUIRE(symbologies >= 1 && (symbologies & ~15360) == 0,
                    "%s: symbologies must be a non-empty subset of 1024 | 2048 | 4096 | 8192 (bit 10 POSTNET, bit 11 PLANET, bit 12 RM4SCC, bit 13 KIX; bit 9 is unassigned, the lower bits are the other three entry points'), got %d",
                    who, symbologies);
        return 0;
    }
};

template <int C>
__global__ __launch_bounds__(DC_THREADS) void pd_decode_kernel(const uint8_t *__restrict__ patches, const int32_t *__restrict__ counts, int cap,
                                                               int ph, int pw, ubd_decode_params P, uint32_t *__restrict__ results)
{
    const int slot = (int)blockIdx.x;                                           // n * cap < 2^31 (checked on the host)
    const int i = slot / cap, j = slot - i * cap;
    if (j >= counts[i]) return;                                                 // j < cap already
    int32_t *tally = (int32_t *)(dc_smem + PD_OFF_TALLY);
    uint32_t *lds_row = (uint32_t *)(dc_smem + PD_OFF_ROW);
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int16_t *store = (int16_t *)(dc_smem + PD_OFF_BARS + wave * PD_WAVE_BARS);
    PdImage<C> I;
    I.src = patches + (int64_t)slot * ph * pw * C;
    I.h = ph; I.w = pw;
    const int S = P.scan_rows, nv = 2 * PD_SYMS * S, asked = P.symbologies >> 10;

    for (int t = tid; t < nv * (PD_SLOT / 8); t += DC_THREADS) ((uint64_t *)dc_smem)[t] = 0;
    if (tid < PD_ROW / 4) lds_row[tid] = tid < 2 ? 0u : 0xFFFFFFFFu;            // the row of "none"; both ordered by the barriers of round 0

    for (int k0 = 0; k0 < S; k0 += DC_WAVES) {
        const int k = k0 + wave;
        const bool on = k < S;                                                  // uniform over the wave
        int32_t *pe;
        int n_edges, l2d0;
        dc_scan_line<C>(I.src, ph, pw, k, S, on, wave, lane, P, dc_smem + PD_TABLE_BYTES, pe, n_edges, l2d0);
        __syncthreads();
        if (on) {                                                               // the candidates
            DcLine L;
            L.e = pe; L.n = n_edges; L.flip = 256 * (pw - 1); L.l2d0 = l2d0;
            const int rk = ((2 * k + 1) * ph) / (2 * S);
            for (int dir = 0; dir < 2; ++dir) {
                L.rev = I.turned = dir == 1;
                const int r0 = dir ? ph - 1 - rk : rk;
                for (int grp = 0; grp < 2; ++grp) {                             // G = 5: POSTNET, PLANET; G = 4: RM4SCC, KIX in direction 0
                    const int G = 5 - grp;
                    int open = (asked >> (2 * grp)) & (grp && dir ? 1 : 3);     // the symbologies of this G that still look for their candidate
                    for (int ib = 0; open && ib < n_edges - 1; ib += 64) {
                        const int c = ib + lane;
                        PdChain ch;
                        int fits = 0;                                           // the open symbologies whose lengths hold the chain's bars
                        if (c < n_edges - 1 && dc_light_to_dark(L, c) &&
                            pd_walk<C, false>(I, r0, dc_edge(L, c), dc_edge(L, c + 1), G, P.window, P.contrast, nullptr, ch)) {
                            for (int b = 0; b < 2; ++b)
                                if ((open >> b & 1) && pd_chars(2 * grp + b, ch.bars)) fits |= 1 << b;
                            if (fits && !pd_quiet<C>(I, L, c, ch, P.quiet)) fits = 0;
                        }
                        unsigned long long todo = __ballot(fits != 0);
                        while (todo && open) {                                  // in rising order, one lane at a time
                            const int src = __ffsll((long long)todo) - 1;
                            todo &= todo - 1;
                            int got = 0;
                            if (lane == src) {
                                pd_walk<C, true>(I, r0, dc_edge(L, c), dc_edge(L, c + 1), G, P.window, P.contrast, store, ch);
                                for (int b = 0; b < 2; ++b)
                                    if (fits >> b & open >> b & 1) {
                                        const int sym = 2 * grp + b, n = pd_chars(sym, ch.bars);
                                        uint8_t *v = (uint8_t *)PdPostal::votes((k * 2 + dir) * PD_SYMS + sym);
                                        if (pd_judge(store, ch.bars, ch.tallest, sym, n, v + 2)) {
                                            v[0] = (uint8_t)n;
                                            v[1] = pd_codes[sym];
                                            got |= 1 << b;
                                        } else {
                                            for (int q = 0; q < PD_SLOT / 4; ++q) ((uint32_t *)v)[q] = 0;
                                        }
                                    }
                            }
                            open &= ~__shfl(got, src);
                        }
                    }
                }
            }
        }
        __syncthreads();                                                        // the next round overwrites the edges
    }

    // the tally: per slot the number of slots with the same payload and the OR of their direction bits
    if (tid < nv) {
        int cnt = 0, mask = 0;
        if (!PdPostal::empty(tid))
            for (int u = 0; u < nv; ++u)
                if (PdPostal::same(tid, u)) { ++cnt; mask |= 1 << ((u / PD_SYMS) & 1); }
        tally[tid] = cnt | mask << 16;
    }
    __syncthreads();
    if (tid == 0) {                                                             // thread 0 turns the row of "none" into the winner's
        int best;
        const int at = dc_winner<PdPostal>(tally, nv, P.min_votes, best);
        if (at >= 0) {
            const uint8_t *win = (const uint8_t *)PdPostal::votes(at);
            uint8_t *bytes = (uint8_t *)lds_row;
            const int t = win[0], sym = at % PD_SYMS;
            bytes[0] = win[1];
            bytes[1] = (uint8_t)best;                                           // <= 2 * 32
            bytes[2] = (uint8_t)(tally[at] >> 16);
            bytes[3] = (uint8_t)t;
            bytes[4] = (uint8_t)(sym != 3);
            bytes[5] = (uint8_t)(sym < 2 ? 5 * t + 2 : sym == 2 ? 4 * t + 2 : 4 * t);
            for (int q = 0; q < t; ++q) bytes[8 + q] = win[2 + q];              // t <= 30
        }
    }
    __syncthreads();
    if (tid < PD_ROW / 4) results[(int64_t)slot * (PD_ROW / 4) + tid] = lds_row[tid];
}

extern "C" int ubd_decode_postal_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                                         const ubd_decode_params *params, uint8_t *results, void *stream)
{
    const char *who = "ubd_decode_postal_patches";
    ubd_decode_params P;
    if (const int rc = dc_check<PdPostal>(who, patches, counts, n, cap, patch_h, patch_w, channels, params, results, P)) return rc;
    const dim3 grid((unsigned)((int64_t)n * cap)), block(DC_THREADS);
    const size_t lds = PD_TABLE_BYTES + dc_lines_bytes(patch_w);                // <= 13440 + 49152 bytes
    if (channels == 3)
        hipLaunchKernelGGL((pd_decode_kernel<3>), grid, block, lds, (hipStream_t)stream, patches, counts, cap, patch_h, patch_w, P, (uint32_t *)results);
    else
        hipLaunchKernelGGL((pd_decode_kernel<1>), grid, block, lds, (hipStream_t)stream, patches, counts, cap, patch_h, patch_w, P, (uint32_t *)results);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
