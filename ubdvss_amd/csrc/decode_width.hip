// Decoding of the object patches, third family: the two-width codes, Interleaved 2 of 5 (ITF, ITF-14), Code 39 and Codabar, out of every
// upright patch that ubd_extract_objects wrote, on the device, so that 128 bytes per object cross to the host instead of the
// patch.  The rules are written out at ubd_decode_width_patches in include/ubd.h and restated, from the rules and not from this
// file, by the numpy oracles tests/width_decode_oracle.py and (Codabar) tests/extra_decode_oracle.py, which this kernel matches
// bit for bit (tests/test_gpu_width_decode.py, tests/test_gpu_extra_decode.py).
// The patterns and the optional checks are those of the public specifications (ISO/IEC 16390, ISO/IEC 16388; Codabar: EN 798).
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_w <= 1024, quiet <= 16).  Edges, runs and
// sums of runs are < 2^18 (decode_scan.h), so
//   narrow or wide: 2 w and lo + hi < 2^19; 2 (least wide) and 3 (greatest narrow) < 2^20;
//   widths of neighbours: 9 S_prev and 8 S < 2^22; Code 39 gap: 12 g < 2^22 and 2 g < 2^19;
//   quiet zones: 4 q, 6 q and 2 q < 2^21 and QZ * S4, QZ * N6, QZ * (space + last bar) <= 16 * 2^18 = 2^22;
//   checks: ITF at most 60 digits of weight 3, <= 1620; Code 39 at most 59 values, <= 42 * 59 = 2478; Codabar 62 values <= 19;
//   Codabar: narrow sums of neighbours 4 * 5 * N and 5 * 5 * N' < 25 * 2^18 < 2^23; gap: 2 * 5 * g < 2^22; quiet zone: 4 q < 2^20.
// No rule divides: every ratio is a comparison of products.
//
// Shape: that of decode_scan.h, which holds the kernel (dc_decode_kernel: prologue, rounds, search, tally, winner rule) and the
// host side of the entry point (dc_decode); decode.hip and decode_text.hip run the same two with their own policies.  This file
// holds the patterns, the group, pair, character and candidate rules (wd_classify .. wd_c39_candidate) and the policy WdWidth.
// A group's runs become a mask of wide runs, the first run the most significant bit; before round 0 the 44 Code 39 words and
// the ten ITF patterns are spread into two LDS tables keyed by that mask (512 and 32 bytes; 0xFF: no pattern), so that a pattern
// costs one LDS byte on the hot path.  A line is searched for three symbologies, so votes go to a table of 6 * scan_rows slots of
// 64 bytes, slot (line, direction, symbology).  A lane walks its candidate without keeping the elements; the lane that votes
// walks it once more and writes count, symbology code and the ASCII elements into its slot.  The tally compares whole slots (16
// dwords: the count in byte 0 and zeroes behind the elements make equal slots equal payloads).  Thread 0 builds the winner's
// 128-byte row in LDS, which leaves as 32 dword stores.  Codabar is the third symbology of a line, with a third table of 128
// bytes keyed by the wide masks of a character's four bars and three spaces.
// LDS: 12288 (votes) + 768 (tally) + 672 (pattern tables) + 128 (row) + at most 49152 (lines) = 63008 bytes.
#include "decode_scan.h"

#define WD_MAX_VOTES (6 * DC_MAX_ROWS)          // slots (line, direction, symbology)
#define WD_SLOT 64                              // bytes of a vote slot: [0] the number of elements, [1] 25 / 39 / 27, [2..] the elements, then zeroes
#define WD_MAX_PAIRS 30
#define WD_MAX_CHARS 60
#define WD_ROW 128                              // bytes of a result row
#define WD_OFF_TALLY (WD_MAX_VOTES * WD_SLOT)
#define WD_OFF_C39 (WD_OFF_TALLY + WD_MAX_VOTES * 4)
#define WD_OFF_ITF (WD_OFF_C39 + 512)
#define WD_OFF_CBR (WD_OFF_ITF + 32)
#define WD_OFF_ROW (WD_OFF_CBR + 128)
#define WD_TABLE_BYTES (WD_OFF_ROW + WD_ROW)    // 13856, a multiple of 16
#define WD_CODE_ITF 25
#define WD_CODE_39 39
#define WD_CODE_CBR 27

// Code 39: the nine runs of a character, a bar first, as a word whose most significant bit is the first bar, 1 = wide; in the
// order of the check values 0..42 (wd_c39_chars), then '*'
__constant__ uint16_t wd_c39_words[44] = {
    0x034, 0x121, 0x061, 0x160, 0x031, 0x130, 0x070, 0x025, 0x124, 0x064, 0x109, 0x049, 0x148, 0x019, 0x118, 0x058, 0x00D, 0x10C, 0x04C, 0x01C, 0x103, 0x043,
    0x142, 0x013, 0x112, 0x052, 0x007, 0x106, 0x046, 0x016, 0x181, 0x0C1, 0x1C0, 0x091, 0x190, 0x0D0, 0x085, 0x184, 0x0C4, 0x0A8, 0x0A2, 0x08A, 0x02A, 0x094};
__constant__ char wd_c39_chars[45] = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%*";
// ITF: the five runs of one colour for the digits 0..9, the same way: nnWWn WnnnW nWnnW WWnnn nnWnW WnWnn nWWnn nnnWW WnnWn nWnWn
__constant__ uint8_t wd_itf_words[10] = {6, 17, 9, 24, 5, 20, 12, 3, 18, 10};

// Codabar: the seven runs of a character, a bar first, the same way; in the order of the values 0..19 (wd_cbr_chars)
__constant__ uint8_t wd_cbr_words[20] = {0x03, 0x06, 0x09, 0x60, 0x12, 0x42, 0x21, 0x24, 0x30, 0x48, 0x0C, 0x18, 0x45, 0x51, 0x54, 0x15, 0x1A, 0x29, 0x0B, 0x0E};
__constant__ char wd_cbr_chars[21] = "0123456789-$:/.+ABCD";

// Narrow or wide over the N runs w[OFF], w[OFF + STRIDE], ..: the mask of the wide runs (the first run is the most significant
// bit), or -1 where no run is wide or 2 * (least wide) < 3 * (greatest narrow).  lo, hi: the least and the greatest run;
// narrow: the sum of the narrow runs.
template <int N, int OFF, int STRIDE, int M>
static __device__ __forceinline__ int wd_classify(const int (&w)[M], int &lo, int &hi, int &narrow)
{
    lo = hi = w[OFF];
#pragma unroll
    for (int k = 1; k < N; ++k) {
        const int v = w[OFF + k * STRIDE];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    int mask = 0, least_wide = 1 << 20, greatest_narrow = 0;                    // every run is < 2^18
    narrow = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int v = w[OFF + k * STRIDE];
        const bool wide = 2 * v > lo + hi;
        mask = mask << 1 | (int)wide;
        if (wide) least_wide = v < least_wide ? v : least_wide;
        else { greatest_narrow = v > greatest_narrow ? v : greatest_narrow; narrow += v; }
    }
    return mask == 0 || 2 * least_wide < 3 * greatest_narrow ? -1 : mask;
}

struct WdPair { int lo_b, hi_b, lo_s, hi_s, s; };  // the least and greatest bar and space of an ITF pair, and its width

// The ITF pair of ten runs between the edges j..j+10: first digit | second digit << 4, or -1.
static __device__ __forceinline__ int wd_pair(const DcLine &L, int j, const uint8_t *itf, WdPair &g)
{
    int w[10], prev = dc_edge(L, j);
    g.s = -prev;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const int next = dc_edge(L, j + k + 1);
        w[k] = next - prev;
        prev = next;
    }
    g.s += prev;
    int nb, ns;
    const int mb = wd_classify<5, 0, 2>(w, g.lo_b, g.hi_b, nb), ms = wd_classify<5, 1, 2>(w, g.lo_s, g.hi_s, ns);
    if ((mb | ms) < 0) return -1;
    const int a = itf[mb], b = itf[ms];                                         // 0xFF: not two wide runs, or no pattern
    return a == 0xFF || b == 0xFF ? -1 : a | b << 4;
}

// The Code 39 character of nine runs between the edges j..j+9: its ASCII code, or -1.  s: its width; n6: the sum of its narrow runs.
static __device__ __forceinline__ int wd_character(const DcLine &L, int j, const uint8_t *c39, int &s, int &n6)
{
    int w[9], prev = dc_edge(L, j);
    s = -prev;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int next = dc_edge(L, j + k + 1);
        w[k] = next - prev;
        prev = next;
    }
    s += prev;
    int lo, hi;
    const int m = wd_classify<9, 0, 1>(w, lo, hi, n6);
    if (m < 0) return -1;
    const int ch = c39[m];                                                      // 0xFF: not three wide runs, or no pattern
    return ch == 0xFF ? -1 : ch;
}

static __device__ __forceinline__ bool wd_not_wide(int w, int lo, int hi) { return lo <= 2 * w && 2 * w <= lo + hi; }

// The ITF candidate that starts at edge i: the number of its digits (6..60), or 0.  WRITE: their ASCII codes go to out.
template <bool WRITE>
static __device__ int wd_itf_candidate(const DcLine &L, int i, int quiet, const uint8_t *itf, uint8_t *out)
{
    if (!dc_light_to_dark(L, i) || i + 4 >= L.n) return 0;
    const int e0 = dc_edge(L, i), e1 = dc_edge(L, i + 1), e2 = dc_edge(L, i + 2), e3 = dc_edge(L, i + 3), e4 = dc_edge(L, i + 4);
    if (i >= 1 && 4 * (e0 - dc_edge(L, i - 1)) < quiet * (e4 - e0)) return 0;
    WdPair first, last;
    int cnt = 0, j = i + 4;
    for (;; j += 10) {                                                          // data before stop: what reads as a pair is one
        if (j + 10 >= L.n) break;
        WdPair g;
        const int v = wd_pair(L, j, itf, g);
        if (v < 0) break;
        if (cnt && (8 * g.s < 7 * last.s || 8 * g.s > 9 * last.s)) break;
        if (cnt == WD_MAX_PAIRS) return 0;
        if (cnt == 0) first = g;
        last = g;
        if (WRITE) {
            out[2 * cnt] = (uint8_t)(48 + (v & 15));
            out[2 * cnt + 1] = (uint8_t)(48 + (v >> 4));
        }
        ++cnt;
    }
    if (cnt < 3) return 0;
    if (!wd_not_wide(e1 - e0, first.lo_b, first.hi_b) || !wd_not_wide(e2 - e1, first.lo_s, first.hi_s) ||
        !wd_not_wide(e3 - e2, first.lo_b, first.hi_b) || !wd_not_wide(e4 - e3, first.lo_s, first.hi_s))
        return 0;
    if (j + 3 >= L.n) return 0;                                                 // the stop: a wide bar, a space and a bar that are not
    const int s0 = dc_edge(L, j), s1 = dc_edge(L, j + 1), s2 = dc_edge(L, j + 2), s3 = dc_edge(L, j + 3);
    if (2 * (s1 - s0) <= last.lo_b + last.hi_b) return 0;
    if (!wd_not_wide(s2 - s1, last.lo_s, last.hi_s) || !wd_not_wide(s3 - s2, last.lo_b, last.hi_b)) return 0;
    if (j + 4 < L.n && 2 * (dc_edge(L, j + 4) - s3) < quiet * (s3 - s1)) return 0;
    return 2 * cnt;
}

// The Code 39 candidate that starts at edge i: the number of its data characters (1..60), or 0.  WRITE: their ASCII codes go to out.
template <bool WRITE>
static __device__ int wd_c39_candidate(const DcLine &L, int i, int quiet, const uint8_t *c39, uint8_t *out)
{
    if (!dc_light_to_dark(L, i) || i + 9 >= L.n) return 0;
    int sp, n6;
    if (wd_character(L, i, c39, sp, n6) != '*') return 0;
    if (i >= 1 && 6 * (dc_edge(L, i) - dc_edge(L, i - 1)) < quiet * n6) return 0;
    int cnt = 0, j = i + 10;
    for (;; j += 10) {
        if (j + 9 >= L.n) return 0;
        const int g = dc_edge(L, j) - dc_edge(L, j - 1);                        // the gap between two characters
        if (n6 > 12 * g || 2 * g > sp) return 0;
        int s;
        const int ch = wd_character(L, j, c39, s, n6);
        if (ch < 0 || 8 * s < 7 * sp || 8 * s > 9 * sp) return 0;
        sp = s;
        if (ch == '*') break;
        if (cnt == WD_MAX_CHARS) return 0;
        if (WRITE) out[cnt] = (uint8_t)ch;
        ++cnt;
    }
    if (cnt == 0) return 0;
    if (j + 10 < L.n && 6 * (dc_edge(L, j + 10) - dc_edge(L, j + 9)) < quiet * n6) return 0;
    return cnt;
}

// The bars (N = 4, OFF = 0) or the spaces (N = 3, OFF = 1) of a Codabar character: the mask of the wide ones, or -1.  The rule
// of wd_classify, and beside it: a colour whose greatest run is less than 1.5 times its least has no wide run (mask 0).
template <int N, int OFF>
static __device__ __forceinline__ int wd_cbr_colour(const int (&w)[7], int &narrow)
{
    int lo, hi;
    const int m = wd_classify<N, OFF, 2>(w, lo, hi, narrow);
    if (m >= 0 || 2 * hi >= 3 * lo) return m;
    narrow = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) narrow += w[OFF + 2 * k];
    return 0;
}

// The Codabar character of seven runs between the edges j..j+7: its value 0..19, or -1.  s: its width; nn: the sum of its narrow
// runs, which are 7 - (the number of its wide runs): five for the values 0..11, four for the others.  Bars and spaces are
// classified apart, as those of an ITF pair are; the table's key is (wide bars) << 3 | (wide spaces).
static __device__ __forceinline__ int wd_cbr_character(const DcLine &L, int j, const uint8_t *cbr, int &s, int &nn)
{
    int w[7], prev = dc_edge(L, j);
    s = -prev;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int next = dc_edge(L, j + k + 1);
        w[k] = next - prev;
        prev = next;
    }
    s += prev;
    int nb, ns;
    const int mb = wd_cbr_colour<4, 0>(w, nb), ms = wd_cbr_colour<3, 1>(w, ns);
    if ((mb | ms) < 0) return -1;
    nn = nb + ns;
    const int v = cbr[mb << 3 | ms];                                            // 0xFF: no pattern
    return v == 0xFF ? -1 : v;
}

static __device__ __forceinline__ int wd_cbr_narrows(int v) { return v < 12 ? 5 : 4; }

// The Codabar candidate that starts at edge i: the number of its characters, start and stop included (3..62), or 0.  WRITE: their
// ASCII codes go to out.
template <bool WRITE>
static __device__ int wd_cbr_candidate(const DcLine &L, int i, int quiet, const uint8_t *cbr, uint8_t *out)
{
    if (!dc_light_to_dark(L, i) || i + 7 >= L.n) return 0;
    int sp, np;
    int v = wd_cbr_character(L, i, cbr, sp, np);
    if (v < 16) return 0;                                                       // A..D
    if (i >= 1 && 4 * (dc_edge(L, i) - dc_edge(L, i - 1)) < quiet * np) return 0;
    if (WRITE) out[0] = (uint8_t)wd_cbr_chars[v];
    int cnt = 1, cp = 4, j = i + 8;
    for (;; j += 8) {
        if (j + 7 >= L.n) return 0;
        const int g = dc_edge(L, j) - dc_edge(L, j - 1);                        // the gap between two characters
        if (np > 2 * cp * g || 2 * g > sp) return 0;
        int s, nn;
        v = wd_cbr_character(L, j, cbr, s, nn);
        if (v < 0) return 0;
        const int c = wd_cbr_narrows(v);
        if (4 * nn * cp < 3 * np * c || 4 * nn * cp > 5 * np * c) return 0;     // the mean narrow runs of neighbours
        sp = s; np = nn; cp = c;
        if (cnt == WD_MAX_CHARS + 1 && v < 16) return 0;
        if (WRITE) out[cnt] = (uint8_t)wd_cbr_chars[v];
        ++cnt;
        if (v >= 16) break;
    }
    if (cnt < 3) return 0;
    if (j + 8 < L.n && 4 * (dc_edge(L, j + 8) - dc_edge(L, j + 7)) < quiet * np) return 0;
    return cnt;
}

// The check value 0..42 of a Code 39 character.
static __device__ __forceinline__ int wd_c39_value(int ch)
{
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'A' && ch <= 'Z') return ch - 'A' + 10;
    return ch == '-' ? 36 : ch == '.' ? 37 : ch == ' ' ? 38 : ch == '$' ? 39 : ch == '/' ? 40 : ch == '+' ? 41 : 42;
}

// Flag bit 0 of a vote slot: the optional check character holds.
static __device__ int wd_check_holds(const uint8_t *slot)
{
    const int t = slot[0];
    int sum = 0;
    if (slot[1] == WD_CODE_ITF) {
        for (int k = 0; k < t - 1; ++k) sum += (slot[2 + k] - 48) * (((t - 1 - k) & 1) ? 3 : 1);
        return (sum + slot[1 + t] - 48) % 10 == 0;
    }
    if (slot[1] == WD_CODE_CBR) {                                               // the values of all characters sum to 0 modulo 16
        for (int k = 0; k < t; ++k) {
            const int ch = slot[2 + k];
            int v = 0;
            for (int q = 0; q < 20; ++q) v = wd_cbr_chars[q] == ch ? q : v;
            sum += v;
        }
        return sum % 16 == 0;
    }
    for (int k = 0; k < t - 1; ++k) sum += wd_c39_value(slot[2 + k]);
    return t >= 2 && sum % 43 == wd_c39_value(slot[1 + t]);
}

static __device__ __forceinline__ bool wd_same(const uint32_t *a, const uint32_t *b)
{
    bool same = true;
#pragma unroll
    for (int q = 0; q < WD_SLOT / 4; ++q) same = same && a[q] == b[q];
    return same;
}

// The policy of dc_decode_kernel (decode_scan.h).  LDS tables: the vote table, the tally, the two pattern tables and the result row.
struct WdWidth {
    typedef uint32_t Word;
    static constexpr int ROW_WORDS = WD_ROW / 4, SYMS = 3, SLOT_BYTES = WD_SLOT, OFF_TALLY = WD_OFF_TALLY, TABLE_BYTES = WD_TABLE_BYTES;

    static __device__ __forceinline__ uint32_t *votes(int u) { return (uint32_t *)dc_smem + u * (WD_SLOT / 4); }
    static __device__ __forceinline__ uint8_t *c39() { return dc_smem + WD_OFF_C39; }
    static __device__ __forceinline__ uint8_t *itf() { return dc_smem + WD_OFF_ITF; }
    static __device__ __forceinline__ uint8_t *cbr() { return dc_smem + WD_OFF_CBR; }
    static __device__ __forceinline__ uint32_t *lds_row() { return (uint32_t *)(dc_smem + WD_OFF_ROW); }

    // the three pattern tables (the masks of a table are distinct, so no two lanes write one entry) and the row of "none"
    static __device__ __forceinline__ void setup(int tid)
    {
        if (tid < (512 + 32 + 128) / 4) ((uint32_t *)c39())[tid] = 0xFFFFFFFFu;
        if (tid < WD_ROW / 4) lds_row()[tid] = tid < 2 ? 0u : 0xFFFFFFFFu;
        __syncthreads();
        if (tid < 44) c39()[wd_c39_words[tid]] = (uint8_t)wd_c39_chars[tid];
        else if (tid >= 64 && tid < 74) itf()[wd_itf_words[tid - 64]] = (uint8_t)(tid - 64);
        else if (tid >= 128 && tid < 148) {
            const int w = wd_cbr_words[tid - 128];                              // b s b s b s b -> b b b b s s s
            const int key = (w >> 6 & 1) << 6 | (w >> 4 & 1) << 5 | (w >> 2 & 1) << 4 | (w & 1) << 3 | (w >> 5 & 1) << 2 | (w >> 3 & 1) << 1 | (w >> 1 & 1);
            cbr()[key] = (uint8_t)(tid - 128);
        }
    }
    static __device__ __forceinline__ int starts(const ubd_decode_params &P, int sym, int n_edges)
    {
        // the shortest symbols: ITF start, three pairs and stop take the edges i .. i + 37; Code 39 '*', one character, '*' and two gaps i .. i + 29;
        // Codabar start, one character, stop and two gaps i .. i + 23 (bit 8)
        if (sym == 2) return P.symbologies & 256 ? n_edges - 23 : 0;
        return (P.symbologies >> (3 + sym)) & 1 ? n_edges - (sym ? 29 : 37) : 0;
    }
    static __device__ __forceinline__ int candidate(const DcLine &L, int i, int sym, int quiet)
    {
        if (sym == 2) return wd_cbr_candidate<false>(L, i, quiet, cbr(), nullptr);
        return sym ? wd_c39_candidate<false>(L, i, quiet, c39(), nullptr) : wd_itf_candidate<false>(L, i, quiet, itf(), nullptr);
    }
    static __device__ __forceinline__ void vote(const DcLine &L, int i, int cnt, int slot)
    {
        uint8_t *s = (uint8_t *)votes(slot);                                    // zeroed before round 0; the slot's index modulo 3 is its symbology
        const int sym = slot % 3;
        s[0] = (uint8_t)cnt;                                                    // <= 62: bytes 2..63
        s[1] = sym == 2 ? WD_CODE_CBR : sym ? WD_CODE_39 : WD_CODE_ITF;
        if (sym == 2) wd_cbr_candidate<true>(L, i, 0, cbr(), s + 2);
        else if (sym) wd_c39_candidate<true>(L, i, 0, c39(), s + 2);            // quiet 0: the quiet-zone tests only reject, and this one is valid
        else wd_itf_candidate<true>(L, i, 0, itf(), s + 2);
    }
    static __device__ __forceinline__ bool empty(int u) { return (votes(u)[0] & 0xFFu) == 0; }
    static __device__ __forceinline__ bool same(int u, int v) { return wd_same(votes(u), votes(v)); }

    // thread 0 turns the row of "none" into the winner's, 32 threads store it
    static __device__ __forceinline__ void emit(const int32_t *tally, int nv, int min_votes, int tid, uint32_t *row)
    {
        if (tid == 0) {
            int best;
            const int at = dc_winner<WdWidth>(tally, nv, min_votes, best);
            if (at >= 0) {
                const uint8_t *win = (const uint8_t *)votes(at);
                uint8_t *bytes = (uint8_t *)lds_row();
                const int t = win[0];
                bytes[0] = win[1];
                bytes[1] = (uint8_t)best;                                       // <= 2 * 32
                bytes[2] = (uint8_t)(tally[at] >> 16);
                bytes[3] = (uint8_t)t;
                bytes[4] = (uint8_t)wd_check_holds(win);
                for (int k = 0; k < t; ++k) bytes[8 + k] = win[2 + k];          // t <= 62
            }
        }
        __syncthreads();                                                        // uniform: every thread of the workgroup is here
        if (tid < WD_ROW / 4) row[tid] = lds_row()[tid];
    }

    static int check_results(const char *who, const void *results)
    {
        UBD_REQUIRE(((uintptr_t)results & 3) == 0, "%s: results must be aligned to 4 bytes", who);
        return 0;
    }
    static int check_symbologies(const char *who, int symbologies)
    {
        UBD_REQUIRE(symbologies >= 1 && (symbologies & ~280) == 0,
                    "%s: symbologies must be a non-empty subset of 8 | 16 | 256 (bit 3 ITF, bit 4 Code 39, bit 8 Codabar; bit 5 is unassigned, the other bits are the other two entry points'), got %d",
                    who, symbologies);
        return 0;
    }
};

extern "C" int ubd_decode_width_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                                        const ubd_decode_params *params, uint8_t *results, void *stream)
{
    return dc_decode<WdWidth>("ubd_decode_width_patches", patches, counts, n, cap, patch_h, patch_w, channels, params, results, stream);
}
