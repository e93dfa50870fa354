// The part of the patch decoders that does not know a symbology.  decode.hip (EAN-13 / UPC-A / EAN-8 / UPC-E), decode_text.hip
// (Code 128, Code 93) and decode_width.hip (ITF, Code 39, Codabar) include it and add a policy struct each (what a policy holds is listed at
// dc_decode_kernel).  decode_postal.hip (POSTNET, PLANET, RM4SCC, KIX) takes the scan front end, dc_winner and dc_check and brings
// a round loop of its own: its candidates are walked on the patch, not on the edge list.  Here are
//   the scan front end: the profile of a scan line, its local threshold and its sub-pixel edges, as the rules at
//     ubd_decode_patches in include/ubd.h define them (dc_scan_line), and the edge list as one reading direction sees it (DcLine);
//   the kernel (dc_decode_kernel): slot prologue, round loop, direction loop, the search for the first valid candidate, the
//     tally, and the rule that picks the winner (dc_winner);
//   the host entry (dc_check, dc_decode): the argument checks; the grid, the LDS size and the launch.
//
// Shape: one workgroup of DC_WAVES waves per patch slot; a workgroup whose slot holds no object returns after one load of
// counts[i].  One wave per scan line, DC_WAVES lines per round.  The four stages of a round (profile, threshold, edges,
// candidates) are separated by workgroup barriers; the round loop and the barriers are uniform over the workgroup, a wave beyond
// the last line idles between them.  Candidates take one lane per start edge, 64 starts a step in rising order; the first step
// that holds a valid candidate ends the search and its lowest lane writes the vote.  Votes go to a fixed table of slots, one per
// (line, direction, symbology), each written by at most one lane, so the result does not depend on the order in which waves run.
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

// The workgroup's LDS: a family's tables (Sym::TABLE_BYTES, the vote table first), then the lines (dc_lines_bytes).
extern __shared__ __align__(16) unsigned char dc_smem[];

// The winner of a tally: the vote slot whose payload has the most votes, -1 if that is less than min_votes or another payload
// has as many.  best: the most votes.  Sym::emit calls it in the threads that need the answer.
template <class Sym>
static __device__ __forceinline__ int dc_winner(const int32_t *tally, int nv, int min_votes, int &best)
{
    int at = -1;
    best = 0;
    for (int u = 0; u < nv; ++u) {
        const int c = tally[u] & 0xffff;
        if (c > best) { best = c; at = u; }
    }
    bool won = at >= 0 && best >= min_votes;
    for (int u = 0; won && u < nv; ++u)
        if ((tally[u] & 0xffff) == best && !Sym::same(at, u)) won = false;      // another payload has as many
    return won ? at : -1;
}

// The decoder of one family.  Sym, the family's policy, holds what differs (its members read and write dc_smem):
//   Word                                the type the result rows are stored as;  ROW_WORDS: their number per row
//   SYMS                                the symbologies a direction of a line is searched for.  Vote slot (k * 2 + dir) * SYMS + sym
//                                       belongs to (line k, direction dir, symbology sym): 2 * SYMS slots per line, and
//                                       (index / SYMS) & 1 is a slot's direction, index % SYMS its symbology
//   SLOT_BYTES                          the bytes of a vote slot, a multiple of 8; the vote table is the front of dc_smem
//   OFF_TALLY, TABLE_BYTES              where the tally's int32 per slot lies, and the bytes of all tables in front of the lines
//   setup(tid)                          fills the family's tables; a barrier in it is uniform (every thread calls it)
//   starts(P, sym, n_edges)             the number of start edges to try, <= 0 when there is none or P leaves the symbology out
//   candidate(L, i, sym, quiet)         the candidate at start edge i, 0 when it is not valid
//   vote(L, i, candidate, slot)         writes the valid candidate into its vote slot
//   empty(u), same(u, v)                vote slot u holds no vote; slots u and v hold the same payload
//   emit(tally, nv, min_votes, tid, row) the result row of dc_winner's slot or of "none"; called by every thread
template <int C, class Sym>
__global__ __launch_bounds__(DC_THREADS) void dc_decode_kernel(const uint8_t *__restrict__ patches, const int32_t *__restrict__ counts, int cap,
                                                               int ph, int pw, ubd_decode_params P, typename Sym::Word *__restrict__ results)
{
    const int slot = (int)blockIdx.x;                                           // n * cap < 2^31 (checked on the host)
    const int i = slot / cap, j = slot - i * cap;
    if (j >= counts[i]) return;                                                 // j < cap already
    int32_t *tally = (int32_t *)(dc_smem + Sym::OFF_TALLY);
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint8_t *src = patches + (int64_t)slot * ph * pw * C;
    const int S = P.scan_rows, nv = 2 * Sym::SYMS * S;

    for (int t = tid; t < nv * (Sym::SLOT_BYTES / 8); t += DC_THREADS) ((uint64_t *)dc_smem)[t] = 0;
    Sym::setup(tid);                                                            // both ordered before the first candidate by the barriers of round 0

    for (int k0 = 0; k0 < S; k0 += DC_WAVES) {
        const int k = k0 + wave;
        const bool on = k < S;                                                  // uniform over the wave
        int32_t *pe;
        int n_edges, l2d0;
        dc_scan_line<C>(src, ph, pw, k, S, on, wave, lane, P, dc_smem + Sym::TABLE_BYTES, pe, n_edges, l2d0);
        __syncthreads();
        if (on) {                                                               // the candidates
            DcLine L;
            L.e = pe; L.n = n_edges; L.flip = 256 * (pw - 1); L.l2d0 = l2d0;
            for (int dir = 0; dir < 2; ++dir) {
                L.rev = dir == 1;
                for (int sym = 0; sym < Sym::SYMS; ++sym) {
                    const int starts = Sym::starts(P, sym, n_edges);
                    for (int ib = 0; ib < starts; ib += 64) {
                        const int c = ib + lane;
                        const auto cand = c < starts ? Sym::candidate(L, c, sym, P.quiet) : 0;
                        const unsigned long long valid = __ballot(cand != 0);
                        if (valid) {                                            // the lowest start index of this (line, direction, symbology)
                            if (lane == __ffsll((long long)valid) - 1) Sym::vote(L, c, cand, (k * 2 + dir) * Sym::SYMS + sym);
                            break;
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
        if (!Sym::empty(tid))
            for (int u = 0; u < nv; ++u)
                if (Sym::same(tid, u)) { ++cnt; mask |= 1 << ((u / Sym::SYMS) & 1); }
        tally[tid] = cnt | mask << 16;
    }
    __syncthreads();
    Sym::emit(tally, nv, P.min_votes, tid, results + (int64_t)slot * Sym::ROW_WORDS);
}

// The argument checks every patch decoder's entry point makes; `who` is its name.  Sym::check_results and Sym::check_symbologies
// hold the family's own rules and return as UBD_REQUIRE does.  P: the caller's copy of *params.
template <class Sym>
static int dc_check(const char *who, const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                    const ubd_decode_params *params, const void *results, ubd_decode_params &P)
{
    UBD_REQUIRE(patches, "%s: patches is null", who);
    UBD_REQUIRE(counts, "%s: counts is null", who);
    UBD_REQUIRE(params, "%s: params is null", who);
    UBD_REQUIRE(results, "%s: results is null", who);
    if (const int rc = Sym::check_results(who, results)) return rc;
    UBD_REQUIRE(n >= 1, "%s: n must be >= 1, got %d", who, n);
    UBD_REQUIRE(cap >= 1, "%s: cap must be >= 1, got %d", who, cap);
    UBD_REQUIRE(patch_h >= 1 && patch_h <= DC_MAX_H, "%s: patch_h must be 1..%d, got %d", who, DC_MAX_H, patch_h);
    UBD_REQUIRE(patch_w >= DC_MIN_W && patch_w <= DC_MAX_W, "%s: patch_w must be %d..%d, got %d", who, DC_MIN_W, DC_MAX_W, patch_w);
    UBD_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, channels);
    P = *params;
    if (const int rc = Sym::check_symbologies(who, P.symbologies)) return rc;
    UBD_REQUIRE(P.scan_rows >= 1 && P.scan_rows <= DC_MAX_ROWS, "%s: scan_rows must be 1..%d, got %d", who, DC_MAX_ROWS, P.scan_rows);
    UBD_REQUIRE(P.band >= 0 && P.band <= 8, "%s: band must be 0..8, got %d", who, P.band);
    UBD_REQUIRE(P.window >= 1 && P.window <= 64, "%s: window must be 1..64, got %d", who, P.window);
    UBD_REQUIRE(P.contrast >= 0 && P.contrast <= 255, "%s: contrast must be 0..255, got %d", who, P.contrast);
    UBD_REQUIRE(P.quiet >= 0 && P.quiet <= 16, "%s: quiet must be 0..16, got %d", who, P.quiet);
    UBD_REQUIRE(P.min_votes >= 1 && P.min_votes <= 2 * P.scan_rows, "%s: min_votes must be 1..2 * scan_rows = %d, got %d", who, 2 * P.scan_rows,
                P.min_votes);
    UBD_REQUIRE((int64_t)n * cap < ((int64_t)1 << 31), "%s: n * cap = %d * %d is not below 2^31", who, n, cap);
    return 0;
}

// The host side of a family's entry point: the checks, the grid, the LDS size and the launch of dc_decode_kernel.
template <class Sym>
static int dc_decode(const char *who, const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                     const ubd_decode_params *params, void *results, void *stream)
{
    ubd_decode_params P;
    if (const int rc = dc_check<Sym>(who, patches, counts, n, cap, patch_h, patch_w, channels, params, results, P)) return rc;
    const dim3 grid((unsigned)((int64_t)n * cap)), block(DC_THREADS);
    const size_t lds = Sym::TABLE_BYTES + dc_lines_bytes(patch_w);              // <= 13856 + 49152 bytes
    typename Sym::Word *rows = (typename Sym::Word *)results;
    if (channels == 3)
        hipLaunchKernelGGL((dc_decode_kernel<3, Sym>), grid, block, lds, (hipStream_t)stream, patches, counts, cap, patch_h, patch_w, P, rows);
    else
        hipLaunchKernelGGL((dc_decode_kernel<1, Sym>), grid, block, lds, (hipStream_t)stream, patches, counts, cap, patch_h, patch_w, P, rows);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
