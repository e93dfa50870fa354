// Decoding of the object patches: the digits of an EAN-13 (UPC-A included) or EAN-8 symbol out of every upright patch that
// ubd_extract_objects wrote, on the device, so that 64 bytes per object cross to the host instead of the patch.  The rules are
// written out at ubd_decode_patches in include/ubd.h and restated, from the rules and not from this file, by the numpy oracle
// tests/decode_oracle.py, which this kernel matches bit for bit (tests/test_gpu_decode.py).  The symbol tables (sets L, G, R,
// the parity words, the checksums) are those of the public EAN/UPC specification (ISO/IEC 15420).
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_w <= 1024, band <= 8, window <= 64).  The
// profile, the threshold and the edges are decode_scan.h's, shared with decode_text.hip: every edge, run and sum of runs is < 2^18.
//   quiet zone: modules * q <= 95 * 2^18 < 2^25 and QZ * St <= 16 * 2^18 = 2^22; guards: 2 * modules * w + St < 191 * 2^18 < 2^26;
//   characters: 14 (w0 + w1) < 2^22, 11 * S4 < 2^22 and |7 (w0 + w2) - S4 (n0 + n2)| < 7 * 2^18 < 2^21.
// The floors of the guard and character rules are taken by comparing products, which is the same thing without the division.
//
// Shape: one workgroup of DC_WAVES waves per patch slot; a workgroup whose slot holds no object returns after one load of
// counts[i].  One wave per scan line, DC_WAVES lines per round.  Per line in LDS: the profile p (int32), over which the edge list
// is later written (p is dead by then), and d (int16).  The four stages of a round (profile, threshold, edges, candidates) are
// separated by workgroup barriers; the round loop and the barriers are uniform over the workgroup, a wave beyond the last line
// idles between them.  The sliding minimum and maximum are the plain loop over the 2R + 1 neighbours: at the defaults that is
// 33 LDS reads per pixel of a 256-pixel line.  Edges are compacted in order, 64 pixels a step, with a ballot and the popcount
// of the lanes below.  Candidates take one lane per start edge, 64 starts a step in rising order; the first step that holds a
// valid candidate ends the search and its lowest lane writes the vote.  Votes go to a fixed table of 4 * scan_rows slots, slot
// (line, direction, symbology), each written by at most one lane, so the result does not depend on the order in which waves run;
// the tally counts, for every slot, the slots that hold the same payload, and lanes 0..15 of wave 0 store the result row.
#include "decode_scan.h"

#define DC_MAX_VOTES (4 * DC_MAX_ROWS)
#define DC_TABLE_BYTES (DC_MAX_VOTES * 8 + DC_MAX_VOTES * 4)       // the vote table (uint64) and the tally's counts (int32)

// The characters by their pair of edge-to-similar-edge distances, key = (E1 - 2) * 4 + (E2 - 2).  Set L, run widths in scan order
// for the digits 0..9, is 3211 2221 2122 1411 1132 1231 1114 1312 1213 3112 (set R the same, set G reversed), so (E1, E2) is
//   L: 0 (5,3)  1 (4,4)  2 (3,3)  3 (5,5)  4 (2,4)  5 (3,5)  6 (2,2)  7 (4,4)  8 (3,3)  9 (4,2)
//   G: 0 (2,3)  1 (3,4)  2 (4,3)  3 (2,5)  4 (5,4)  5 (4,5)  6 (5,2)  7 (3,4)  8 (4,3)  9 (3,2)
// every one of the 16 keys belongs to one set, and only 1 / 7 and 2 / 8 share theirs.  The tables are immediates, not memory.
#define DC_KEY_DIGIT 0x3406512951293406ull      // nibble `key`: the digit, the lower one of a pair
#define DC_KEY_IS_G 0x5A5Au                     // bit `key`: the key belongs to set G
#define DC_KEY_IS_PAIR 0x0660u                  // bit `key`: digit and digit + 6 share the key
// n0 + n2 of a pair's patterns: L 2221 / 2122 -> 4 and 1312 / 1213 -> 2; G 1222 / 2212 -> 3 and 2131 / 3121 -> 5
// the parity words of the six left characters of an EAN-13 for the first digits 0..9, six bits each (bit 5 = first character,
// 1 = set G): LLLLLL LLGLGG LLGGLG LLGGGL LGLLGG LGGLLG LGGGLL LGLGLG LGLGGL LGGLGL
#define DC_PARITY_WORDS ((0x00ull) | (0x0Bull << 6) | (0x0Dull << 12) | (0x0Eull << 18) | (0x13ull << 24) | (0x19ull << 30) | \
                         (0x1Cull << 36) | (0x15ull << 42) | (0x16ull << 48) | (0x1Aull << 54))

// floor((14 a + s4) / (2 s4)) without a division: it is >= k exactly when 14 a >= (2k - 1) s4; 0: outside 2..5
static __device__ __forceinline__ int dc_distance(int a, int s4)
{
    const int t = 14 * a;
    if (t < 3 * s4 || t >= 11 * s4) return 0;
    return 2 + (t >= 5 * s4) + (t >= 7 * s4) + (t >= 9 * s4);
}

// One character of four runs, edge to similar edge; with_g: sets L and G, else set L (= R).  false: no pattern or a tie.
// The patterns that match (E1, E2) are at most two; between the two of a pair the smaller |7 (w0 + w2) - S4 (n0 + n2)| decides.
static __device__ __forceinline__ bool dc_character(int w0, int w1, int w2, int w3, bool with_g, int &digit, int &is_g)
{
    const int s4 = w0 + w1 + w2 + w3;
    if (s4 <= 0) return false;
    const int e1 = dc_distance(w0 + w1, s4), e2 = dc_distance(w1 + w2, s4);
    if (!e1 || !e2) return false;
    const int key = (e1 - 2) * 4 + (e2 - 2);
    is_g = (DC_KEY_IS_G >> key) & 1;
    if (is_g && !with_g) return false;
    digit = (int)((DC_KEY_DIGIT >> (4 * key)) & 15ull);
    if ((DC_KEY_IS_PAIR >> key) & 1) {
        const int odd = 7 * (w0 + w2);
        int lower = odd - s4 * (is_g ? 3 : 4), upper = odd - s4 * (is_g ? 5 : 2);
        lower = lower < 0 ? -lower : lower;
        upper = upper < 0 ? -upper : upper;
        if (lower == upper) return false;
        if (upper < lower) digit += 6;
    }
    return true;
}

// The candidate that starts at edge i: its payload key, or 0.  sym: 0 EAN-13, 1 EAN-8.
// key = code << 52 | 13 nibbles, digit k at bits 4 * (12 - k), an unused place is 15
static __device__ uint64_t dc_candidate(const DcLine &L, int i, int sym, int quiet)
{
    const int runs = sym ? 43 : 59, modules = sym ? 67 : 95, half = sym ? 4 : 6;
    if (!dc_light_to_dark(L, i)) return 0;
    const int e0 = dc_edge(L, i), e_end = dc_edge(L, i + runs), st = e_end - e0;
    if (st <= 0) return 0;
    if (i >= 1 && modules * (e0 - dc_edge(L, i - 1)) < quiet * st) return 0;
    if (i + runs + 1 < L.n && modules * (dc_edge(L, i + runs + 1) - e_end) < quiet * st) return 0;
    const int centre = 3 + 4 * half;
    for (int g = 0; g < 11; ++g) {                                              // start guard, centre guard, end guard
        const int j = i + (g < 3 ? g : g < 8 ? centre + g - 3 : runs - 11 + g);
        const int w = dc_edge(L, j + 1) - dc_edge(L, j);
        if (2 * modules * w < st || 2 * modules * w >= 3 * st) return 0;        // (2 modules w + St) / (2 St) == 1, without the division
    }
    int sum = 0, parity = 0, last = 0;
    uint64_t digits = 0;
    for (int c = 0; c < 2 * half; ++c) {
        const bool right = c >= half;
        const int r = i + 3 + 4 * c + (right ? 5 : 0);
        const int a0 = dc_edge(L, r), a1 = dc_edge(L, r + 1), a2 = dc_edge(L, r + 2), a3 = dc_edge(L, r + 3), a4 = dc_edge(L, r + 4);
        int digit = 0, is_g = 0;
        if (!dc_character(a1 - a0, a2 - a1, a3 - a2, a4 - a3, sym == 0 && !right, digit, is_g)) return 0;
        if (!right) parity = parity << 1 | is_g;
        const int idx = sym ? c : c + 1;                                        // the digit's place in the payload
        if (c == 2 * half - 1) last = digit;
        else sum += digit * (((idx & 1) != 0) == (sym == 0) ? 3 : 1);           // EAN-13: odd places weigh 3; EAN-8: even places
        digits = digits << 4 | (uint64_t)digit;
    }
    if (sym == 0) {
        int first = -1;
#pragma unroll
        for (int k = 0; k < 10; ++k)
            if ((int)((DC_PARITY_WORDS >> (6 * k)) & 63ull) == parity) first = k;
        if (first < 0) return 0;
        sum += first;
        digits |= (uint64_t)first << 48;
    } else {
        digits = digits << 20 | 0xFFFFFull;
    }
    if ((10 - sum % 10) % 10 != last) return 0;
    return (uint64_t)(sym ? 8 : 13) << 52 | digits;
}

template <int C>
__global__ __launch_bounds__(DC_THREADS) void decode_kernel(const uint8_t *__restrict__ patches, const int32_t *__restrict__ counts, int cap,
                                                            int ph, int pw, ubd_decode_params P, int32_t *__restrict__ results)
{
    extern __shared__ __align__(8) unsigned char dc_smem[];
    const int slot = (int)blockIdx.x;                                           // n * cap < 2^31 (checked on the host)
    const int i = slot / cap, j = slot - i * cap;
    if (j >= counts[i]) return;                                                 // j < cap already
    uint64_t *votes = (uint64_t *)dc_smem;
    int32_t *tally = (int32_t *)(dc_smem + DC_MAX_VOTES * 8);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const uint8_t *src = patches + (int64_t)slot * ph * pw * C;
    const int S = P.scan_rows, nv = 4 * S;

    for (int t = (int)threadIdx.x; t < nv; t += DC_THREADS) votes[t] = 0;       // ordered before the first vote by the barriers of round 0

    for (int k0 = 0; k0 < S; k0 += DC_WAVES) {
        const int k = k0 + wave;
        const bool on = k < S;                                                  // uniform over the wave
        int32_t *pe;
        int n_edges, l2d0;
        dc_scan_line<C>(src, ph, pw, k, S, on, wave, lane, P, dc_smem + DC_TABLE_BYTES, pe, n_edges, l2d0);
        __syncthreads();
        if (on) {                                                               // the candidates
            DcLine L;
            L.e = pe; L.n = n_edges; L.flip = 256 * (pw - 1); L.l2d0 = l2d0;
            for (int dir = 0; dir < 2; ++dir) {
                L.rev = dir == 1;
                for (int sym = 0; sym < 2; ++sym) {
                    if (!((P.symbologies >> sym) & 1)) continue;
                    const int starts = n_edges - (sym ? 43 : 59);               // start i needs the edges i .. i + runs
                    for (int ib = 0; ib < starts; ib += 64) {
                        const int c = ib + lane;
                        const uint64_t key = c < starts ? dc_candidate(L, c, sym, P.quiet) : 0;
                        const unsigned long long valid = __ballot(key != 0);
                        if (valid) {                                            // the lowest start index of this (line, direction, symbology)
                            if (lane == __ffsll((long long)valid) - 1) votes[(k * 2 + dir) * 2 + sym] = key;
                            break;
                        }
                    }
                }
            }
        }
        __syncthreads();                                                        // the next round overwrites the edges
    }

    // the tally: per slot the number of slots with the same payload and the OR of their direction bits
    if ((int)threadIdx.x < nv) {
        const uint64_t key = votes[threadIdx.x];
        int cnt = 0, mask = 0;
        if (key)
            for (int u = 0; u < nv; ++u)
                if (votes[u] == key) { ++cnt; mask |= 1 << ((u >> 1) & 1); }
        tally[threadIdx.x] = cnt | mask << 16;
    }
    __syncthreads();
    if (wave == 0) {                                                            // every lane walks the table (LDS broadcasts)
        int best = 0, at = -1;
        for (int u = 0; u < nv; ++u) {
            const int c = tally[u] & 0xffff;
            if (c > best) { best = c; at = u; }
        }
        uint64_t key = at >= 0 ? votes[at] : 0;
        for (int u = 0; u < nv; ++u)
            if (key && (tally[u] & 0xffff) == best && votes[u] != key) { key = 0; break; }   // another payload has as many
        if (best < P.min_votes) key = 0;
        if (lane < 16) {
            int v;
            if (lane == 0) v = (int)(key >> 52);
            else if (lane == 1) v = key ? best : 0;
            else if (lane == 2) v = key ? tally[at] >> 16 : 0;
            else {
                const int nib = key ? (int)((key >> (4 * (15 - lane))) & 15ull) : 15;
                v = nib == 15 ? -1 : nib;
            }
            results[(int64_t)slot * 16 + lane] = v;
        }
    }
}

extern "C" int ubd_decode_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                                  const ubd_decode_params *params, int32_t *results, void *stream)
{
    UBD_REQUIRE(patches, "ubd_decode_patches: patches is null");
    UBD_REQUIRE(counts, "ubd_decode_patches: counts is null");
    UBD_REQUIRE(params, "ubd_decode_patches: params is null");
    UBD_REQUIRE(results, "ubd_decode_patches: results is null");
    UBD_REQUIRE(n >= 1, "ubd_decode_patches: n must be >= 1, got %d", n);
    UBD_REQUIRE(cap >= 1, "ubd_decode_patches: cap must be >= 1, got %d", cap);
    UBD_REQUIRE(patch_h >= 1 && patch_h <= DC_MAX_H, "ubd_decode_patches: patch_h must be 1..%d, got %d", DC_MAX_H, patch_h);
    UBD_REQUIRE(patch_w >= DC_MIN_W && patch_w <= DC_MAX_W, "ubd_decode_patches: patch_w must be %d..%d, got %d", DC_MIN_W, DC_MAX_W, patch_w);
    UBD_REQUIRE(channels == 1 || channels == 3, "ubd_decode_patches: channels must be 1 or 3, got %d", channels);
    const ubd_decode_params P = *params;
    UBD_REQUIRE(P.symbologies >= 1 && P.symbologies <= 3, "ubd_decode_patches: symbologies must be 1..3 (bit 0 EAN-13, bit 1 EAN-8; bit 2, Code 128, is read by ubd_decode_text_patches), got %d", P.symbologies);
    UBD_REQUIRE(P.scan_rows >= 1 && P.scan_rows <= DC_MAX_ROWS, "ubd_decode_patches: scan_rows must be 1..%d, got %d", DC_MAX_ROWS, P.scan_rows);
    UBD_REQUIRE(P.band >= 0 && P.band <= 8, "ubd_decode_patches: band must be 0..8, got %d", P.band);
    UBD_REQUIRE(P.window >= 1 && P.window <= 64, "ubd_decode_patches: window must be 1..64, got %d", P.window);
    UBD_REQUIRE(P.contrast >= 0 && P.contrast <= 255, "ubd_decode_patches: contrast must be 0..255, got %d", P.contrast);
    UBD_REQUIRE(P.quiet >= 0 && P.quiet <= 16, "ubd_decode_patches: quiet must be 0..16, got %d", P.quiet);
    UBD_REQUIRE(P.min_votes >= 1 && P.min_votes <= 2 * P.scan_rows, "ubd_decode_patches: min_votes must be 1..2 * scan_rows = %d, got %d",
                2 * P.scan_rows, P.min_votes);
    UBD_REQUIRE((int64_t)n * cap < ((int64_t)1 << 31), "ubd_decode_patches: n * cap = %d * %d is not below 2^31", n, cap);
    const dim3 grid((unsigned)((int64_t)n * cap)), block(DC_THREADS);
    const size_t lds = DC_TABLE_BYTES + dc_lines_bytes(patch_w);                          // <= 1536 + 49152 bytes
    if (channels == 3)
        hipLaunchKernelGGL(decode_kernel<3>, grid, block, lds, (hipStream_t)stream, patches, counts, cap, patch_h, patch_w, P, results);
    else
        hipLaunchKernelGGL(decode_kernel<1>, grid, block, lds, (hipStream_t)stream, patches, counts, cap, patch_h, patch_w, P, results);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
