// Decoding of the object patches: the digits of an EAN-13 (UPC-A included), EAN-8 or UPC-E symbol out of every upright patch that
// ubd_extract_objects wrote, on the device, so that 64 bytes per object cross to the host instead of the patch.  The rules are
// written out at ubd_decode_patches in include/ubd.h and restated, from the rules and not from this file, by the numpy oracle
// tests/decode_oracle.py, which this kernel matches bit for bit (tests/test_gpu_decode.py).  The symbol tables (sets L, G, R,
// the parity words, the checksums) are those of the public EAN/UPC specification (ISO/IEC 15420).
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_w <= 1024, band <= 8, window <= 64).  The
// profile, the threshold and the edges are decode_scan.h's, shared with decode_text.hip: every edge, run and sum of runs is < 2^18.
//   quiet zone: modules * q <= 95 * 2^18 < 2^25 and QZ * St <= 16 * 2^18 = 2^22; guards: 2 * modules * w + St < 191 * 2^18 < 2^26;
//   UPC-E: its trailing quiet zone 51 q < 2^24 against 5 St < 2^21; its check sum <= 3 * 1 + 9 * (1 + 3 + 1 + 3 + 1 + 3) = 111;
//   characters: 14 (w0 + w1) < 2^22, 11 * S4 < 2^22 and |7 (w0 + w2) - S4 (n0 + n2)| < 7 * 2^18 < 2^21.
// The floors of the guard and character rules are taken by comparing products, which is the same thing without the division.
//
// Shape: that of decode_scan.h, which holds the kernel (dc_decode_kernel: prologue, rounds, search, tally, winner rule) and the
// host side of the entry point (dc_decode); decode_text.hip runs the same two with its own policy.  This file holds the EAN
// tables, the character and candidate rules (dc_distance, dc_character, dc_candidate) and the policy DcRetail.  The sliding
// minimum and maximum of the scan are the plain loop over the 2R + 1 neighbours: at the defaults that is 33 LDS reads per pixel
// of a 256-pixel line.  A line is searched for three symbologies, so votes go to a table of 6 * scan_rows slots, slot (line,
// direction, symbology), each a 56-bit payload key (0: no vote); the tally counts, for every slot, the slots that hold the same
// key, and lanes 0..15 of wave 0 store the result row.  LDS: 1536 (votes) + 768 (tally) + at most 49152 (lines) = 51456 bytes.
// A mask without UPC-E runs an instance of the kernel that searches two symbologies: 4 * scan_rows slots, 50688 bytes.
#include "decode_scan.h"


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

// the parity words of the six characters of a UPC-E of number system 0 for the check digits 0..9, the same way (number system 1
// has their complements): GGGLLL GGLGLL GGLLGL GGLLLG GLGGLL GLLGGL GLLLGG GLGLGL GLGLLG GLLGLG
#define DC_UPCE_WORDS ((0x38ull) | (0x34ull << 6) | (0x32ull << 12) | (0x31ull << 18) | (0x2Cull << 24) | (0x26ull << 30) | \
                       (0x23ull << 36) | (0x2Aull << 42) | (0x29ull << 48) | (0x25ull << 54))
#define DC_UPCE_RUNS 33
#define DC_UPCE_MODULES 51
#define DC_UPCE_QUIET 5                         // modules of the trailing quiet zone a UPC-E has whatever `quiet` says

// The UPC-E candidate that starts at edge i: its payload key, or 0.  Start guard of 3 runs, six characters of the sets L and G,
// end guard of 6 runs; the parity word gives number system and check digit, which the UPC-A number the six digits stand for
// must confirm.  key = 6 << 52 | number system, d1..d6, check digit and five unused places, as dc_candidate lays them out
static __device__ uint64_t dc_upce_candidate(const DcLine &L, int i, int quiet)
{
    if (!dc_light_to_dark(L, i)) return 0;
    const int e0 = dc_edge(L, i), e_end = dc_edge(L, i + DC_UPCE_RUNS), st = e_end - e0;
    if (st <= 0) return 0;
    if (i >= 1 && DC_UPCE_MODULES * (e0 - dc_edge(L, i - 1)) < quiet * st) return 0;
    if (i + DC_UPCE_RUNS + 1 < L.n) {                                           // behind it at least 5 modules and at least `quiet`
        const int q = DC_UPCE_MODULES * (dc_edge(L, i + DC_UPCE_RUNS + 1) - e_end);
        if (q < quiet * st || q < DC_UPCE_QUIET * st) return 0;
    }
    for (int g = 0; g < 9; ++g) {                                               // start guard, end guard
        const int j = i + (g < 3 ? g : DC_UPCE_RUNS - 9 + g);
        const int w = dc_edge(L, j + 1) - dc_edge(L, j);
        if (2 * DC_UPCE_MODULES * w < st || 2 * DC_UPCE_MODULES * w >= 3 * st) return 0;
    }
    int parity = 0, d[6];
    uint64_t digits = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int r = i + 3 + 4 * c;
        const int a0 = dc_edge(L, r), a1 = dc_edge(L, r + 1), a2 = dc_edge(L, r + 2), a3 = dc_edge(L, r + 3), a4 = dc_edge(L, r + 4);
        int is_g = 0;
        d[c] = 0;
        if (!dc_character(a1 - a0, a2 - a1, a3 - a2, a4 - a3, true, d[c], is_g)) return 0;
        parity = parity << 1 | is_g;
        digits = digits << 4 | (uint64_t)d[c];
    }
    int ns = -1, check = 0;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const int word = (int)((DC_UPCE_WORDS >> (6 * k)) & 63ull);
        if (word == parity) { ns = 0; check = k; }
        if ((word ^ 63) == parity) { ns = 1; check = k; }
    }
    if (ns < 0) return 0;
    // the UPC-A number: number system, ten digits (weights 3 1 3 1 .. from the number system on), check digit
    int sum = 3 * ns + d[0] + 3 * d[1];
    if (d[5] <= 2) sum += d[5] + 3 * d[2] + d[3] + 3 * d[4];                    // d1 d2 d6 0 0 0 0 d3 d4 d5
    else if (d[5] == 3) sum += d[2] + d[3] + 3 * d[4];                          // d1 d2 d3 0 0 0 0 0 d4 d5
    else if (d[5] == 4) sum += d[2] + 3 * d[3] + 3 * d[4];                      // d1 d2 d3 d4 0 0 0 0 0 d5
    else sum += d[2] + 3 * d[3] + d[4] + 3 * d[5];                              // d1 d2 d3 d4 d5 0 0 0 0 d6
    if ((10 - sum % 10) % 10 != check) return 0;
    return (uint64_t)6 << 52 | (uint64_t)ns << 48 | digits << 24 | (uint64_t)check << 20 | 0xFFFFFull;
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

// The policy of dc_decode_kernel (decode_scan.h).  LDS tables: the vote table, one payload key per slot (0: no vote), then the tally.
// UPCE: the mask holds bit 6 and a line is searched for a third symbology.  A mask without it runs the instance of two, whose
// code and tables are those from before UPC-E: with the third symbology in the one kernel the older masks took 4 us more a call.
template <bool UPCE>
struct DcRetail {
    typedef int32_t Word;
    static constexpr int SYMS = UPCE ? 3 : 2, MAX_VOTES = 2 * SYMS * DC_MAX_ROWS;
    static constexpr int ROW_WORDS = 16, SLOT_BYTES = 8, OFF_TALLY = MAX_VOTES * 8, TABLE_BYTES = MAX_VOTES * 8 + MAX_VOTES * 4;   // the vote table (uint64) and the tally's counts (int32)

    static __device__ __forceinline__ uint64_t *votes() { return (uint64_t *)dc_smem; }
    static __device__ __forceinline__ void setup(int) {}
    static __device__ __forceinline__ int starts(const ubd_decode_params &P, int sym, int n_edges)
    {
        if (UPCE && sym == 2) return n_edges - DC_UPCE_RUNS;                    // bit 6 is set
        return (P.symbologies >> sym) & 1 ? n_edges - (sym ? 43 : 59) : 0;      // start i needs the edges i .. i + runs
    }
    static __device__ __forceinline__ uint64_t candidate(const DcLine &L, int i, int sym, int quiet)
    {
        return UPCE && sym == 2 ? dc_upce_candidate(L, i, quiet) : dc_candidate(L, i, sym, quiet);
    }
    static __device__ __forceinline__ void vote(const DcLine &, int, uint64_t key, int slot) { votes()[slot] = key; }
    static __device__ __forceinline__ bool empty(int u) { return votes()[u] == 0; }
    static __device__ __forceinline__ bool same(int u, int v) { return votes()[u] == votes()[v]; }

    // every lane of wave 0 walks the table (LDS broadcasts); lanes 0..15 store the row
    static __device__ __forceinline__ void emit(const int32_t *tally, int nv, int min_votes, int tid, int32_t *row)
    {
        if (tid >= 64) return;
        int best;
        const int at = dc_winner<DcRetail<UPCE>>(tally, nv, min_votes, best);
        const uint64_t key = at >= 0 ? votes()[at] : 0;
        if (tid < 16) {
            int v;
            if (tid == 0) v = (int)(key >> 52);
            else if (tid == 1) v = key ? best : 0;
            else if (tid == 2) v = key ? tally[at] >> 16 : 0;
            else {
                const int nib = key ? (int)((key >> (4 * (15 - tid))) & 15ull) : 15;
                v = nib == 15 ? -1 : nib;
            }
            row[tid] = v;
        }
    }

    static int check_results(const char *, const void *) { return 0; }
    static int check_symbologies(const char *who, int symbologies)
    {
        UBD_REQUIRE(symbologies >= 1 && (symbologies & ~67) == 0,
                    "%s: symbologies must be a non-empty subset of 1 | 2 | 64 (bit 0 EAN-13, bit 1 EAN-8, bit 6 UPC-E; the other bits are the other two entry points'), got %d",
                    who, symbologies);
        return 0;
    }
};

extern "C" int ubd_decode_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                                  const ubd_decode_params *params, int32_t *results, void *stream)
{
    if (params && (params->symbologies & 64))
        return dc_decode<DcRetail<true>>("ubd_decode_patches", patches, counts, n, cap, patch_h, patch_w, channels, params, results, stream);
    return dc_decode<DcRetail<false>>("ubd_decode_patches", patches, counts, n, cap, patch_h, patch_w, channels, params, results, stream);
}
