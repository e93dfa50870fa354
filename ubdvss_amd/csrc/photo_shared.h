// What the photometric kernels (photometric.hip) and the mask-blended stages (noise_alpha.hip) share: the 64 x 16 tile and thread
// shape, the byte tile's LDS pitches, the clamps, the reflect-101 fold and the Keys weights.
#pragma once
#include "common.h"

#define PH_MAX_SIDE 16384
#define PH_THREADS 256
#define PH_PX 4                 // pixels per lane
#define PH_TW 64
#define PH_TH 16
#define PH_HALO 4
#define PH_MAX_TAP (13 * 16384)

__device__ __forceinline__ int ph_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// clamp(v >> n, 0, 255) as a clamp of v followed by a logical shift of the non-negative value: the same number (the shift is
// monotonic), and two instructions (v_med3_i32, v_lshrrev_b32) whose result needs no masking when the bytes are packed
template <int N> __device__ __forceinline__ int ph_shift_clamp(int v)
{
    const int top = (256 << N) - 1;
    v = v < 0 ? 0 : (v > top ? top : v);
    return (int)((unsigned)v >> N);
}

__device__ __forceinline__ int ph_reflect(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

template <int C> struct ph_tile_shape {
    static constexpr int IN_PITCH = C == 3 ? 57 * 4 : 19 * 4;           // bytes; >= 3 + (PH_TW + 2 PH_HALO) C
    static constexpr int IN_DWORDS = C == 3 ? 56 : 19;                  // dwords that can hold source bytes of one row
    static constexpr int T_PITCH = PH_TW * C + 2;                       // ushorts: 97 / 33 dwords
};

// Keys bicubic weights (a = -3/4) at phase k / 32 in Q17: exact integers that sum to 131072
__device__ __forceinline__ void ph_keys(int k, int wgt[4])
{
    const int u = 32 - k;
    wgt[0] = -3 * k * u * u;
    wgt[1] = 5 * k * k * k - 288 * k * k + 131072;
    wgt[2] = 5 * u * u * u - 288 * u * u + 131072;
    wgt[3] = -3 * u * k * k;
}
