// Decoding of the object patches, second family: the text of a Code 128 / GS1-128 or Code 93 symbol out of every upright patch that
// ubd_extract_objects wrote, on the device, so that 128 bytes per object cross to the host instead of the patch.  The rules are
// written out at ubd_decode_text_patches in include/ubd.h and restated, from the rules and not from this file, by the numpy
// oracle tests/text_decode_oracle.py, which this kernel matches bit for bit (tests/test_gpu_text_decode.py).  The patterns, the
// code sets and the modulo-103 check are those of the public Code 128 specification (ISO/IEC 15417); the 48 patterns of Code 93
// and its two modulo-47 check characters are those of its public specification (AIM USS-93).
//
// Integer arithmetic only, and every intermediate fits an int32 at the limits (patch_w <= 1024, quiet <= 16).  Edges, runs and
// sums of runs are < 2^18 (decode_scan.h), so
//   characters: 22 (w + w') < 22 * 2^18 < 2^23 and 15 S < 2^22; bar sum: 11 (w0 + w2 + w4) < 2^22, S V <= 8 * 2^18 = 2^21, and
//     twice their difference < 2^23; widths of neighbours: 5 S_prev < 2^21; stop bar: 22 b < 2^23;
//   quiet zone: 11 q < 2^22 and QZ * S <= 16 * 2^18 = 2^22;
//   check: start + sum k d_k over at most 61 values (the check value is taken out again at the stop)
//     <= 105 + 102 * (61 * 62 / 2) = 192987;
//   Code 93: characters 18 (w + w') < 2^23 and 9 S < 2^22, bar sum 9 (w0 + w2 + w4) < 2^22 and S V <= 6 * 2^18; termination bar 18 b
//     < 2^23; quiet zone 9 q < 2^22; checks: at most 61 values <= 46 of weight <= 20, <= 56120.
// No division is left: the floors of the character, stop-bar and quiet-zone rules are taken by comparing products.
//
// Shape: that of decode_scan.h, which holds the kernel (dc_decode_kernel: prologue, rounds, search, tally, winner rule) and the
// host side of the entry point (dc_decode); decode.hip runs the same two with its own policy.  This file holds the patterns,
// the character and candidate rules (tx_distance .. tx_expand, tx_same) and the policy TxText.  Before round 0 the 107 patterns
// (one hex digit per run) are spread into a table of 6^4 entries in LDS, key ((E0 - 2) * 6 + (E1 - 2)) * 6 .. -> value | V << 8
// (0xFFFF: no pattern); the 107 keys are distinct, so no two lanes write one entry.  Of the lanes of a search step almost every
// one ends at the start-character test.  A lane walks its candidate without keeping the values (count, running check sum and
// last value are enough to accept it); the lane that votes decodes the characters once more and writes count and values into the
// 64-byte vote slot of (line, direction).  The tally compares whole slots (16 dwords; the count in byte 0 and zeroes behind the
// values make equal slots equal payloads).  Thread 0 expands the winner's text into a 128-byte row in LDS, which leaves as 32
// dword stores.  Code 93 is the second symbology of a line: its 48 patterns go to a table of 4^4 entries beside the first (its
// distances are 2..5), and a lane that finds start, characters, stop, termination bar and quiet zones in place walks the
// characters a second time for the two check sums, whose weights count from the right and so need the length first.
// LDS: 8192 (votes) + 512 (tally) + 2592 + 512 (key tables) + 128 (row) + at most 49152 (lines) = 61088 bytes; the mask 4 runs an
// instance of the kernel that searches Code 128 alone, with 4096 + 256 + 2592 + 128 + at most 49152 = 56224 bytes.
#include "decode_scan.h"

#define TX_SLOT 64                              // bytes of a vote slot: [0] the number of values, [1..] the values, then zeroes
                                                // (Code 93: the start value 47, data, C and K; a Code 128 begins with 103..105)
#define TX_MAX_VALUES 62                        // start + 60 data + check
#define TX_KEYS 1296                            // 6^4
#define TX_ROW 128                              // bytes of a result row
#define TX_KEYS93 256                           // 4^4
#define TX_STAR93 47                            // start and stop of a Code 93
#define TX_MAX_VALUES93 62                      // 60 data, C and K
#define TX_START_A 103
#define TX_STOP 106

// run widths for the values 0..106, a bar first, one hex digit per run; 103 / 104 / 105 are Start A / B / C, 106 is the first
// six runs of the stop
__constant__ uint32_t tx_patterns[107] = {
    0x212222, 0x222122, 0x222221, 0x121223, 0x121322, 0x131222, 0x122213, 0x122312, 0x132212, 0x221213, 0x221312, 0x231212,
    0x112232, 0x122132, 0x122231, 0x113222, 0x123122, 0x123221, 0x223211, 0x221132, 0x221231, 0x213212, 0x223112, 0x312131,
    0x311222, 0x321122, 0x321221, 0x312212, 0x322112, 0x322211, 0x212123, 0x212321, 0x232121, 0x111323, 0x131123, 0x131321,
    0x112313, 0x132113, 0x132311, 0x211313, 0x231113, 0x231311, 0x112133, 0x112331, 0x132131, 0x113123, 0x113321, 0x133121,
    0x313121, 0x211331, 0x231131, 0x213113, 0x213311, 0x213131, 0x311123, 0x311321, 0x331121, 0x312113, 0x312311, 0x332111,
    0x314111, 0x221411, 0x431111, 0x111224, 0x111422, 0x121124, 0x121421, 0x141122, 0x141221, 0x112214, 0x112412, 0x122114,
    0x122411, 0x142112, 0x142211, 0x241211, 0x221114, 0x413111, 0x241112, 0x134111, 0x111242, 0x121142, 0x121241, 0x114212,
    0x124112, 0x124211, 0x411212, 0x421112, 0x421211, 0x212141, 0x214121, 0x412121, 0x111143, 0x111341, 0x131141, 0x114113,
    0x114311, 0x411113, 0x411311, 0x113141, 0x114131, 0x311141, 0x411131, 0x211412, 0x211214, 0x211232, 0x233111};

// Code 93: run widths for the values 0..47 the same way: the digits, A..Z, - . space $ / + %, the shifts ($) (%) (/) (+), start / stop
__constant__ uint32_t tx_patterns93[48] = {
    0x131112, 0x111213, 0x111312, 0x111411, 0x121113, 0x121212, 0x121311, 0x111114, 0x131211, 0x141111, 0x211113, 0x211212,
    0x211311, 0x221112, 0x221211, 0x231111, 0x112113, 0x112212, 0x112311, 0x122112, 0x132111, 0x111123, 0x111222, 0x111321,
    0x121122, 0x131121, 0x212112, 0x212211, 0x211122, 0x211221, 0x221121, 0x222111, 0x112122, 0x112221, 0x122121, 0x123111,
    0x121131, 0x311112, 0x311211, 0x321111, 0x112131, 0x113121, 0x211131, 0x121221, 0x312111, 0x311121, 0x122211, 0x111141};

// floor((22 a + s) / (2 s)) - 2 without a division: the floor is >= m exactly when 22 a >= (2m - 1) s; -1: outside 2..7
static __device__ __forceinline__ int tx_distance(int a, int s)
{
    const int t = 22 * a;
    if (t < 3 * s || t >= 15 * s) return -1;
    return (t >= 5 * s) + (t >= 7 * s) + (t >= 9 * s) + (t >= 11 * s) + (t >= 13 * s);
}

// One character of six runs between the edges e[0..6]: its value 0..106, or -1.
static __device__ __forceinline__ int tx_character(const int (&e)[7], const uint16_t *keys)
{
    const int s = e[6] - e[0];
    if (s <= 0) return -1;
    const int d0 = tx_distance(e[2] - e[0], s), d1 = tx_distance(e[3] - e[1], s), d2 = tx_distance(e[4] - e[2], s),
              d3 = tx_distance(e[5] - e[3], s);
    if ((d0 | d1 | d2 | d3) < 0) return -1;
    const int entry = keys[((d0 * 6 + d1) * 6 + d2) * 6 + d3];
    if (entry == 0xFFFF) return -1;
    int off = 11 * ((e[1] - e[0]) + (e[3] - e[2]) + (e[5] - e[4])) - s * (entry >> 8);
    off = off < 0 ? -off : off;
    if (2 * off >= 3 * s) return -1;
    return entry & 0xFF;
}

// Code 93: floor((18 a + s) / (2 s)) - 2 the same way; -1: outside 2..5
static __device__ __forceinline__ int tx_distance93(int a, int s)
{
    const int t = 18 * a;
    if (t < 3 * s || t >= 11 * s) return -1;
    return (t >= 5 * s) + (t >= 7 * s) + (t >= 9 * s);
}

// One Code 93 character of six runs between the edges e[0..6]: its value 0..47, or -1.
static __device__ __forceinline__ int tx_character93(const int (&e)[7], const uint16_t *keys)
{
    const int s = e[6] - e[0];
    if (s <= 0) return -1;
    const int d0 = tx_distance93(e[2] - e[0], s), d1 = tx_distance93(e[3] - e[1], s), d2 = tx_distance93(e[4] - e[2], s),
              d3 = tx_distance93(e[5] - e[3], s);
    if ((d0 | d1 | d2 | d3) < 0) return -1;
    const int entry = keys[((d0 * 4 + d1) * 4 + d2) * 4 + d3];
    if (entry == 0xFFFF) return -1;
    int off = 9 * ((e[1] - e[0]) + (e[3] - e[2]) + (e[5] - e[4])) - s * (entry >> 8);
    off = off < 0 ? -off : off;
    if (2 * off >= 3 * s) return -1;
    return entry & 0xFF;
}

static __device__ __forceinline__ void tx_load(const DcLine &L, int j, int (&e)[7])
{
#pragma unroll
    for (int k = 0; k < 7; ++k) e[k] = dc_edge(L, j + k);
}

// The candidate that starts at edge i: the number of its values (start, data, check: 3..62), or 0.
static __device__ int tx_candidate(const DcLine &L, int i, int quiet, const uint16_t *keys)
{
    if (!dc_light_to_dark(L, i) || i + 6 >= L.n) return 0;
    int e[7];
    tx_load(L, i, e);
    int v = tx_character(e, keys);
    if (v < TX_START_A || v > TX_START_A + 2) return 0;
    int sp = e[6] - e[0];
    if (i >= 1 && 11 * (e[0] - dc_edge(L, i - 1)) < quiet * sp) return 0;
    int sum = v, cnt = 1, last = 0, s, j = i + 6;
    for (;; j += 6) {
        if (j + 6 >= L.n) return 0;
        tx_load(L, j, e);
        s = e[6] - e[0];
        if (4 * s < 3 * sp || 4 * s > 5 * sp) return 0;
        v = tx_character(e, keys);
        if (v < 0 || (v >= TX_START_A && v <= TX_START_A + 2)) return 0;
        if (v == TX_STOP) break;
        if (cnt == TX_MAX_VALUES) return 0;
        sum += cnt * v;                                                         // the data weight k of value number cnt is cnt
        last = v;
        ++cnt;
        sp = s;
    }
    if (j + 7 >= L.n) return 0;
    const int e7 = dc_edge(L, j + 7), bar = 22 * (e7 - e[6]);
    if (bar < 3 * s || bar >= 5 * s) return 0;                                  // (22 b + S) / (2 S) == 2
    if (j + 8 < L.n && 11 * (dc_edge(L, j + 8) - e7) < quiet * s) return 0;
    if (cnt < 3) return 0;
    sum -= (cnt - 1) * last;                                                    // the last value is the check, not data
    return sum % 103 == last ? cnt : 0;
}

// The Code 93 candidate that starts at edge i: the number of its values behind the start (data, C, K: 3..62), or 0.
static __device__ int tx_candidate93(const DcLine &L, int i, int quiet, const uint16_t *keys)
{
    if (!dc_light_to_dark(L, i) || i + 6 >= L.n) return 0;
    int e[7];
    tx_load(L, i, e);
    if (tx_character93(e, keys) != TX_STAR93) return 0;
    int sp = e[6] - e[0];
    if (i >= 1 && 9 * (e[0] - dc_edge(L, i - 1)) < quiet * sp) return 0;
    int cnt = 0, s, j = i + 6;
    for (;; j += 6) {
        if (j + 6 >= L.n) return 0;
        tx_load(L, j, e);
        s = e[6] - e[0];
        if (4 * s < 3 * sp || 4 * s > 5 * sp) return 0;
        const int v = tx_character93(e, keys);
        if (v < 0) return 0;
        if (v == TX_STAR93) break;
        if (cnt == TX_MAX_VALUES93) return 0;
        ++cnt;
        sp = s;
    }
    if (j + 7 >= L.n) return 0;
    const int e7 = dc_edge(L, j + 7), bar = 18 * (e7 - e[6]);
    if (bar < s || bar >= 3 * s) return 0;                                      // (18 b + S) / (2 S) == 1
    if (j + 8 < L.n && 9 * (dc_edge(L, j + 8) - e7) < quiet * s) return 0;
    if (cnt < 3) return 0;
    // C over the data, weights 1..20 cycling from the right; K over the data and C, weights 1..15
    const int D = cnt - 2;
    int c_sum = 0, k_sum = 0, c_val = 0, k_val = 0;
    for (int c = 0; c < cnt; ++c) {
        tx_load(L, i + 6 + 6 * c, e);
        const int v = tx_character93(e, keys);
        if (c < D) c_sum += v * ((D - 1 - c) % 20 + 1);
        if (c <= D) k_sum += v * ((D - c) % 15 + 1);
        if (c == D) c_val = v;
        k_val = v;
    }
    return c_sum % 47 == c_val && k_sum % 47 == k_val ? cnt : 0;
}

// The values of the valid candidate at edge i into its vote slot (zeroed before round 0).
static __device__ void tx_write_values(const DcLine &L, int i, int cnt, const uint16_t *keys, uint8_t *slot)
{
    slot[0] = (uint8_t)cnt;
    for (int c = 0; c < cnt; ++c) {                                             // cnt <= 62: bytes 1..62
        int e[7];
        tx_load(L, i + 6 * c, e);
        slot[1 + c] = (uint8_t)tx_character(e, keys);
    }
}

static __device__ void tx_write_values93(const DcLine &L, int i, int cnt, const uint16_t *keys, uint8_t *slot)
{
    slot[0] = (uint8_t)(cnt + 1);
    for (int c = 0; c <= cnt; ++c) {                                            // cnt <= 62: bytes 1..63
        int e[7];
        tx_load(L, i + 6 * c, e);
        slot[1 + c] = (uint8_t)tx_character93(e, keys);
    }
}

// The text elements of the values in a vote slot into row[8..]; returns their number T (<= 2 * 60).
static __device__ int tx_expand(const uint8_t *slot, uint8_t *text)
{
    const int cnt = slot[0];
    int cur = slot[1] - TX_START_A, t = 0;                                      // 0 / 1 / 2: set A / B / C
    bool shift = false;
    for (int k = 2; k < cnt; ++k) {                                             // slot[2 .. cnt - 1] are the data values
        const int v = slot[k];
        if (cur == 2) {
            if (v < 100) { text[t++] = (uint8_t)(48 + v / 10); text[t++] = (uint8_t)(48 + v % 10); }
            else if (v == 102) text[t++] = 0xF1;
            else cur = v == 100 ? 1 : 0;
            continue;
        }
        const int code = shift ? 1 - cur : cur;                                 // a shifted character is read in the other set
        shift = false;
        if (v < 96) text[t++] = (uint8_t)(code == 0 ? (v < 64 ? v + 32 : v - 64) : v + 32);
        else if (v == 96) text[t++] = 0xF3;
        else if (v == 97) text[t++] = 0xF2;
        else if (v == 98) shift = true;
        else if (v == 99) cur = 2;
        else if (v == 100) { if (code == 0) cur = 1; else text[t++] = 0xF4; }
        else if (v == 101) { if (code == 0) text[t++] = 0xF4; else cur = 0; }
        else text[t++] = 0xF1;
    }
    return t;
}

static __device__ __forceinline__ bool tx_same(const uint32_t *a, const uint32_t *b)
{
    bool same = true;
#pragma unroll
    for (int q = 0; q < TX_SLOT / 4; ++q) same = same && a[q] == b[q];
    return same;
}

// The policy of dc_decode_kernel (decode_scan.h).  LDS tables: the vote table, the tally, the key table(s) and the result row.
// C93: the mask holds bit 7 and a line is searched for a second symbology.  The mask 4 runs the instance of one, whose code
// and tables (7072 bytes) are those from before Code 93: with both in the one kernel the mask 4 took 4 us more a call.
template <bool C93>
struct TxText {
    typedef uint32_t Word;
    static constexpr int SYMS = C93 ? 2 : 1, MAX_VOTES = 2 * SYMS * DC_MAX_ROWS;                  // slots (line, direction, symbology)
    static constexpr int OFF_TALLY = MAX_VOTES * TX_SLOT, OFF_KEYS = OFF_TALLY + MAX_VOTES * 4, OFF_KEYS93 = OFF_KEYS + TX_KEYS * 2;
    static constexpr int OFF_ROW = OFF_KEYS93 + (C93 ? TX_KEYS93 * 2 : 0), TABLE_BYTES = OFF_ROW + TX_ROW;   // 11936 or 7072, multiples of 16
    static constexpr int ROW_WORDS = TX_ROW / 4, SLOT_BYTES = TX_SLOT;

    static __device__ __forceinline__ uint32_t *votes(int u) { return (uint32_t *)dc_smem + u * (TX_SLOT / 4); }
    static __device__ __forceinline__ uint16_t *keys() { return (uint16_t *)(dc_smem + OFF_KEYS); }
    static __device__ __forceinline__ uint16_t *keys93() { return (uint16_t *)(dc_smem + OFF_KEYS93); }
    static __device__ __forceinline__ uint32_t *lds_row() { return (uint32_t *)(dc_smem + OFF_ROW); }

    // the key tables of the 107 and the 48 patterns (one behind the other) and the row of "none"
    static __device__ __forceinline__ void setup(int tid)
    {
        for (int t = tid; t < (TX_KEYS + (C93 ? TX_KEYS93 : 0)) / 2; t += DC_THREADS) ((uint32_t *)keys())[t] = 0xFFFFFFFFu;
        if (tid < TX_ROW / 4) lds_row()[tid] = tid < 2 ? 0u : 0xFFFFFFFFu;
        __syncthreads();
        if (tid < 107) {
            const uint32_t p = tx_patterns[tid];
            int n[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) n[k] = (int)((p >> (4 * (5 - k))) & 15u);
            const int key = (((n[0] + n[1] - 2) * 6 + (n[1] + n[2] - 2)) * 6 + (n[2] + n[3] - 2)) * 6 + (n[3] + n[4] - 2);   // sums of two widths: 2..7 for these patterns
            keys()[key] = (uint16_t)(tid | (n[0] + n[2] + n[4]) << 8);
        } else if (C93 && tid >= 128 && tid < 128 + 48) {
            const uint32_t p = tx_patterns93[tid - 128];
            int n[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) n[k] = (int)((p >> (4 * (5 - k))) & 15u);
            const int key = (((n[0] + n[1] - 2) * 4 + (n[1] + n[2] - 2)) * 4 + (n[2] + n[3] - 2)) * 4 + (n[3] + n[4] - 2);   // sums of two widths: 2..5 for these patterns
            keys93()[key] = (uint16_t)((tid - 128) | (n[0] + n[2] + n[4]) << 8);
        }
    }
    static __device__ __forceinline__ int starts(const ubd_decode_params &P, int sym, int n_edges)
    {
        // Code 128: start, one data, check and stop take the edges i .. i + 25 (bit 2); Code 93: start, one data, C, K and stop i .. i + 31 (bit 7)
        if (!C93) return n_edges - 25;
        return sym ? n_edges - 31 : (P.symbologies & 4 ? n_edges - 25 : 0);
    }
    static __device__ __forceinline__ int candidate(const DcLine &L, int i, int sym, int quiet)
    {
        return C93 && sym ? tx_candidate93(L, i, quiet, keys93()) : tx_candidate(L, i, quiet, keys());
    }
    static __device__ __forceinline__ void vote(const DcLine &L, int i, int cnt, int slot)
    {
        if (C93 && (slot & 1)) tx_write_values93(L, i, cnt, keys93(), (uint8_t *)votes(slot));   // the slot's lowest bit is its symbology
        else tx_write_values(L, i, cnt, keys(), (uint8_t *)votes(slot));
    }
    static __device__ __forceinline__ bool empty(int u) { return (votes(u)[0] & 0xFFu) == 0; }
    static __device__ __forceinline__ bool same(int u, int v) { return tx_same(votes(u), votes(v)); }

    // thread 0 turns the row of "none" into the winner's, 32 threads store it
    static __device__ __forceinline__ void emit(const int32_t *tally, int nv, int min_votes, int tid, uint32_t *row)
    {
        if (tid == 0) {
            int best;
            const int at = dc_winner<TxText<C93>>(tally, nv, min_votes, best);
            if (at >= 0) {
                const uint8_t *win = (const uint8_t *)votes(at);
                uint8_t *bytes = (uint8_t *)lds_row();
                const int cnt = win[0];
                bytes[1] = (uint8_t)best;                                       // <= 2 * 32
                bytes[2] = (uint8_t)(tally[at] >> 16);
                if (C93 && win[1] == TX_STAR93) {                                      // Code 93: an element per data value, the shifts as 0xE1..0xE4
                    const int D = cnt - 3;
                    bytes[0] = 93;
                    bytes[3] = bytes[5] = (uint8_t)D;                           // <= 60: bytes 8..67
                    bytes[4] = 0;
                    bytes[6] = win[cnt - 1];
                    bytes[7] = win[cnt];
                    for (int k = 0; k < D; ++k) {
                        const int v = win[2 + k];
                        bytes[8 + k] = (uint8_t)(v < 10 ? 48 + v : v < 36 ? 55 + v : v < 43 ? "-. $/+%"[v - 36] : 0xE1 + v - 43);
                    }
                } else {
                    bytes[0] = 128;
                    bytes[3] = (uint8_t)tx_expand(win, bytes + 8);              // T <= 120: bytes 8..127
                    bytes[4] = win[2] == 102 ? 1 : 0;                           // the first data character is FNC1
                    bytes[5] = (uint8_t)(cnt - 2);
                    bytes[6] = win[1];
                    bytes[7] = win[cnt];
                }
            }
        }
        __syncthreads();                                                        // uniform: every thread of the workgroup is here
        if (tid < TX_ROW / 4) row[tid] = lds_row()[tid];
    }

    static int check_results(const char *who, const void *results)
    {
        UBD_REQUIRE(((uintptr_t)results & 3) == 0, "%s: results must be aligned to 4 bytes", who);
        return 0;
    }
    static int check_symbologies(const char *who, int symbologies)
    {
        UBD_REQUIRE(symbologies == 4 || symbologies == 128 || symbologies == 132,
                    "%s: symbologies must be 4, 128 or 132 (bit 2 Code 128, bit 7 Code 93; the other bits are the other two entry points'), got %d", who,
                    symbologies);
        return 0;
    }
};

extern "C" int ubd_decode_text_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                                       const ubd_decode_params *params, uint8_t *results, void *stream)
{
    if (params && (params->symbologies & 128))
        return dc_decode<TxText<true>>("ubd_decode_text_patches", patches, counts, n, cap, patch_h, patch_w, channels, params, results, stream);
    return dc_decode<TxText<false>>("ubd_decode_text_patches", patches, counts, n, cap, patch_h, patch_w, channels, params, results, stream);
}
