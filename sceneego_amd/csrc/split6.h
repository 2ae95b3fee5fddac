// Float32 products as six bf16 products on v_mfma_f32_16x16x32_bf16 (the bf16 matrix pipe: 16x the f32 MFMA rate and not the
// vector ALU port the f32 MFMA issues on).  Stated once for the direct-GEMM launches of the V2V side that have a split form.
//
// Arithmetic: an activation x = a + b + c and a weight w = p + q + r, every part a bf16 value taken with round to nearest even:
//     a = bf16(x), b = bf16(x - a), c = bf16(x - a - b)          (the subtractions are exact in float32)
// so |b| <= 2^-8 |x|, |c| <= 2^-16 |x| and |x - a - b - c| <= 2^-27 |x| (three signed parts of 8 significant bits cover the 24 bits
// of x: barring underflow the split is exact).  Of the nine part products the six largest are
// taken - ap, aq, bp, ar, cp, bq - each exact in the MFMA's float32 product, summed in its float32 accumulator; the three dropped
// ones (br, cq, cr) total <= 2^-23 |x| |w|, twice the rounding of ONE float32 product and far below the accumulated rounding of the
// K = 32 ... 3456 terms of these launches.
//
// Operand layout of v_mfma_f32_16x16x32_bf16 (bf16_common.h): lane l holds the 8 consecutive k = 8 (l >> 4) .. + 7 of row (A) or
// column (B) l & 15 as 16 bytes; D: lane l holds rows 4 (l >> 4) .. + 3 of column l & 15 - the D map of v_mfma_f32_16x16x4_f32, so
// a split form keeps its float32 form's epilogue.  Weights are split once, at pack time (conv3d_pack.h: se_split6_value, three
// planes in A-fragment order); activations on their way into the operand registers or into LDS.
#pragma once
#include "bf16_common.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The three planes of one operand fragment: p[0] the leading parts (a / p), p[1] the middle (b / q), p[2] the last (c / r).
struct Split6Frag { u16x8 p[3]; };

// Two float32 values -> their three bf16 parts, packed pairwise (v_cvt_pk_bf16_f32 is round to nearest even).
__device__ __forceinline__ void se_split3_pair(float x0, float x1, unsigned (&part)[3]) {
    f32x2 v = {x0, x1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bf16x2 h = __builtin_convertvector(v, bf16x2);
        part[k] = __builtin_bit_cast(unsigned, h);
        if (k < 2) v -= __builtin_convertvector(h, f32x2);
    }
}

// 8 consecutive k of a row / column (two float32 quads) -> one operand fragment
__device__ __forceinline__ Split6Frag se_split3_x8(f32x4 lo, f32x4 hi) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    unsigned w[4][3];
    se_split3_pair(lo.x, lo.y, w[0]);
    se_split3_pair(lo.z, lo.w, w[1]);
    se_split3_pair(hi.x, hi.y, w[2]);
    se_split3_pair(hi.z, hi.w, w[3]);
    Split6Frag f;
#pragma unroll
    for (int k = 0; k < 3; ++k) f.p[k] = __builtin_bit_cast(u16x8, (u32x4){w[0][k], w[1][k], w[2][k], w[3][k]});
    return f;
}

// The six-product group, smallest class first (2^-16: bq, cp, ar; 2^-8: bp, aq; then ap): plane of the weight fragment, plane of
// the activation fragment.  acc += w . x over a fragment's 32 k is
//     for (k < SE_S6_PRODUCTS) acc = mfma_bf16(w.p[SE_S6_W[k]], x.p[SE_S6_X[k]], acc);
// a kernel with several accumulators walks the products in the OUTER loop, so that consecutive MFMAs go to different accumulators.
constexpr int SE_S6_PRODUCTS = 6;
constexpr int SE_S6_W[SE_S6_PRODUCTS] = {1, 0, 2, 0, 1, 0};
constexpr int SE_S6_X[SE_S6_PRODUCTS] = {1, 2, 0, 1, 0, 0};
