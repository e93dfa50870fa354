// fp32 products as TWO-PIECE fp16 SPLIT PRODUCTS under a power-of-two scale, on v_mfma_f32_16x16x32_f16 (fp32 accumulate): the
// helpers of the Winograd layer's default form (wino6.hip).  split3.h is the three-piece bf16 form of the same products.
//
// An fp16 value carries 11 significand bits, so two pieces carry 22 (23 with the sign of the second):
//     h1 = f16(x),  h2 = f16(x - h1)        both rounded to NEAREST;  x - h1 is exact in fp32
//     |x - (h1 + h2)| <= 2^-22 |x| + 2^-25  (the second term: h2 below 2^-14 is an fp16 subnormal with a 2^-24 quantum)
// and a product of two such values keeps h1 g1 + h1 g2 + h2 g1; the dropped h2 g2 is <= 2^-22 of the product's bound.
// fp16's exponent range (65504 down to 2^-24) is what the SCALE is for: x is multiplied by a power of two s chosen from the
// largest magnitude of the values that share one accumulation, so that the largest lands in [2^top, 2^(top + 1)); the result is
// multiplied by 1 / s.  Both multiplications are exact, so results are bit-for-bit homogeneous under powers of two.
// The scale rule and the rounding are plain C++ that the host compiler builds too (tests/test_wino6_f16_pack_host.py): the
// weight pack uses exactly this text; the layer kernel uses the rule as it stands and the hardware's conversions
// (v_cvt_pk_f16_f32, round to nearest even) for the rounding.
#pragma once

#if defined(__HIPCC__)
#define SPLIT2H_FN __host__ __device__ __forceinline__
#else
#include <cstring>
#define SPLIT2H_FN inline
#endif

SPLIT2H_FN unsigned split2h_bits(float v)
{
#if defined(__HIPCC__)
    return __builtin_bit_cast(unsigned, v);
#else
    unsigned u; memcpy(&u, &v, 4); return u;
#endif
}
SPLIT2H_FN float split2h_float(unsigned u)
{
#if defined(__HIPCC__)
    return __builtin_bit_cast(float, u);
#else
    float v; memcpy(&v, &u, 4); return v;
#endif
}

// Exponent clamps of the scale rule (biased fp32 exponents of the largest magnitude).  Below the low clamp the scale stops growing
// (values that small keep their 22 bits for another 16 binades and then fade into fp16's subnormals); the low clamps of the two
// factors are chosen so that the product of the two inverse scales, 2^(lo_s - top_s - 127) 2^(lo_w - top_w - 127) = 2^-149, is still
// an fp32 number.  Inf / NaN inputs (exponent 255) are treated as the largest finite binade: the scale stays finite and normal.
#define SPLIT2H_SAMPLE_TOP 13      // rows of the input transform: |T| s in [2^13, 2^14), |V| <= 2 |T|, so |V s| < 2^15 < 65504
#define SPLIT2H_SAMPLE_LO 40
#define SPLIT2H_WEIGHT_TOP 12      // max |U| t in [2^12, 2^13)
#define SPLIT2H_WEIGHT_LO 90

// maxbits: the bit pattern of the largest |value| (sign clear).  Returns the bits of s = 2^(top - e) and of 1 / s, where e is the
// (clamped) exponent of that value; s = 1 for an all-zero set.  Both are normal numbers for the clamps above.
SPLIT2H_FN void split2h_scale(unsigned maxbits, int top, int lo, unsigned &s_bits, unsigned &inv_bits)
{
    int e = (int)(maxbits >> 23);
    e = e < lo ? lo : (e > 254 ? 254 : e);
    const bool zero = maxbits == 0u;
    s_bits = zero ? 0x3f800000u : (unsigned)(254 + top - e) << 23;
    inv_bits = zero ? 0x3f800000u : (unsigned)(e - top) << 23;
}

// the value of the fp16 number nearest to x (ties to even; subnormals kept; past 65520 infinity), as a float
SPLIT2H_FN float split2h_round_f16(float x)
{
    const unsigned u = split2h_bits(x), sign = u & 0x80000000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return x;                                  // Inf, NaN
    if (a < 0x38800000u) {                                           // |x| < 2^-14: multiples of 2^-24
        const float m = split2h_float(a);
        const float r = (m + 0.5f) - 0.5f;                           // the sum lies in [0.5, 1): its ulp is 2^-24, ties to even
        return split2h_float(split2h_bits(r) | sign);
    }
    unsigned r = a + 0xfffu + ((a >> 13) & 1u);                      // 10 mantissa bits, ties to even
    r &= 0xffffe000u;
    if (r >= 0x47800000u) r = 0x7f800000u;                           // 65536 and up
    return split2h_float(r | sign);
}

// the two pieces of an (already scaled) value
SPLIT2H_FN void split2h_pieces(float xs, float &h1, float &h2)
{
    h1 = split2h_round_f16(xs);
    h2 = split2h_round_f16(xs - h1);
}

#if defined(__HIPCC__)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the fp16 bit pattern of a float that IS an fp16 value (what split2h_round_f16 returns): the conversion is exact
__device__ __forceinline__ unsigned split2h_f16_bits(float h) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)h); }

// Both pieces of two scaled values as packed k-slot pairs {lo half: a, hi half: b}: v_cvt_pk_f16_f32, 2 x v_cvt_f32_f16 (the high
// half by SDWA), v_pk_add_f32 (or two v_sub_f32), v_cvt_pk_f16_f32 -- five or six instructions for two values.
__device__ __forceinline__ void split2h_pair(float a, float b, unsigned &p1, unsigned &p2)
{
    const f32x2 v = {a, b};
    const f16x2 h1 = __builtin_convertvector(v, f16x2);
    const f32x2 r = v - __builtin_convertvector(h1, f32x2);
    const f16x2 h2 = __builtin_convertvector(r, f16x2);
    p1 = __builtin_bit_cast(unsigned, h1);
    p2 = __builtin_bit_cast(unsigned, h2);
}
// the lane's six k-slots (channels 4q .. 4q+3, 16+2q, 17+2q; slots 6, 7 zero) as the two operand quads
__device__ __forceinline__ void split2h_6(f32x4 a, f32x2 b, u32x4 &P1, u32x4 &P2)
{
    unsigned p1[3], p2[3];
    split2h_pair(a[0], a[1], p1[0], p2[0]);
    split2h_pair(a[2], a[3], p1[1], p2[1]);
    split2h_pair(b[0], b[1], p1[2], p2[2]);
    P1 = (u32x4){p1[0], p1[1], p1[2], 0u};
    P2 = (u32x4){p2[0], p2[1], p2[2], 0u};
}
// The same pieces with the residual taken by a mixed-precision fma: v_fma_mix_f32 computes a b + c in fp32 with each operand fp32
// or one HALF of a packed fp16 register, so x - h1 reads h1 where v_cvt_pk_f16_f32 left it and the two conversions back to fp32
// go: v_cvt_pk_f16_f32, 2 x v_fma_mix_f32, v_cvt_pk_f16_f32 -- four instructions for two values.  x 1 - h1 is exact, as x - h1 is:
// the same bits.  v_fma_mix_f32 issues at the rate of the conversions (4.4 cycles per instruction and SIMD at two waves); the forms
// that round to fp16 themselves (v_fma_mixlo_f16 / v_fma_mixhi_f16, which would save the last conversion too) take 8.4 and lose
// (tools/ubench/valu_ops.hip, profiles/r16_ubench_valu_mix.txt).
// `one` is a 1.0f that the caller hides from the optimiser (an empty asm): with a visible 1 the fma folds to a subtraction, which
// hipcc builds from two conversions again.  The empty asm here makes the packed h1 opaque, so that its halves are read in place
// (op_sel) instead of being recomputed.  Plain C++ otherwise: hipcc's scheduler and hazard recogniser see every instruction (wino6.hip).
__device__ __forceinline__ void split2h_pair_m(float a, float b, float one, unsigned &p1, unsigned &p2)
{
    const f32x2 v = {a, b};
    f16x2 h1 = __builtin_convertvector(v, f16x2);
    asm("" : "+v"(h1));
    const f32x2 r = {__builtin_fmaf(a, one, -(float)h1[0]), __builtin_fmaf(b, one, -(float)h1[1])};
    const f16x2 h2 = __builtin_convertvector(r, f16x2);
    p1 = __builtin_bit_cast(unsigned, h1);
    p2 = __builtin_bit_cast(unsigned, h2);
}
__device__ __forceinline__ void split2h_6m(f32x4 a, f32x2 b, float one, u32x4 &P1, u32x4 &P2)
{
    unsigned p1[3], p2[3];
    split2h_pair_m(a[0], a[1], one, p1[0], p2[0]);
    split2h_pair_m(a[2], a[3], one, p1[1], p2[1]);
    split2h_pair_m(b[0], b[1], one, p1[2], p2[2]);
    P1 = (u32x4){p1[0], p1[1], p1[2], 0u};
    P2 = (u32x4){p2[0], p2[1], p2[2], 0u};
}
__device__ __forceinline__ f32x4 mfma16h(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
#endif
