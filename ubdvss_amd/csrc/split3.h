// fp32 products as EXACT THREE-WAY bf16 SPLIT PRODUCTS on v_mfma_f32_16x16x32_bf16 (fp32 accumulate): the helpers shared by
// the Winograd layer (wino6.hip) and the fp32 stem's pointwise products (stem123.h).
//
// Every fp32 value v is the exact sum of three bf16 values obtained by truncation,
//     v = v1 + v2 + v3,   v1 = hi16(v),  v2 = hi16(v - v1),  v3 = hi16(v - v1 - v2)       (8 + 8 + 8 = 24 significand bits),
// so a product of two fp32 values is the sum of nine bf16 x bf16 products (each exact in fp32).  The six with i + j <= 4 are kept;
// the three dropped ones are <= 2^-24 of the product -- the size of the rounding of an fp32 multiply.  WHICH six are kept is pinned for the
// stem by tests/test_gpu_exact32.py: bit equality on inputs on which each kept product is live and each dropped one zero (tests/exact_cases.py).  K = 24 channels fit one
// K = 32 step: lane (m, q) holds the k-slots 0..5 of k-group q = channels 4q .. 4q+3, 16+2q, 17+2q (slots 6, 7 zero).
// All arithmetic is plain C++ on vector types (no inline asm): hipcc's scheduler and hazard recogniser see every instruction
// (wino6.hip records what an asm v_add_f32 next to an MFMA result did).
#pragma once

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// residual of the truncation to bf16: v - hi16(v), exact
__device__ __forceinline__ f32x4 resid(f32x4 v) { return v - __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, v) & 0xffff0000u); }
__device__ __forceinline__ f32x2 resid(f32x2 v) { return v - __builtin_bit_cast(f32x2, __builtin_bit_cast(u32x2, v) & 0xffff0000u); }
// {hi16(lo), hi16(hi)} as one dword of two bf16 k-slots
__device__ __forceinline__ unsigned pack_hi(float lo, float hi) { return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u); }
__device__ __forceinline__ u32x4 pack6(f32x4 a, f32x2 b) { return (u32x4){pack_hi(a[0], a[1]), pack_hi(a[2], a[3]), pack_hi(b[0], b[1]), 0u}; }
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// the three pieces of one value, as the high halves of three dwords (what pack_hi reads): the pack-time form of the split
__device__ __forceinline__ void split3_bits(float v, unsigned (&b)[3])
{
    b[0] = __float_as_uint(v) & 0xffff0000u;
    const float r1 = v - __uint_as_float(b[0]);
    b[1] = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(b[1]);
    b[2] = __float_as_uint(r2) & 0xffff0000u;
}
