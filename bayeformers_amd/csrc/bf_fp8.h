// bf_fp8.h — the e4m3fn row converters shared by the two FP8 row formats: the centred kept weights of
// bf_gemm_skinny_fp8.hip (include/bayeformers_amd_fp8.h) and the KV-cache rows of bf_kv8.hip / bf_attention_decode.hip
// (include/bayeformers_amd_kv8.h).  A row is D bytes of OCP E4M3 (finite-only, bias 7) over one power-of-two scale 2^e.
#pragma once
#include "bf_common.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

constexpr int kFp8ExpClamp = 64;  // |e| of a row's scale 2^e

__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }

// The row's exponent: the smallest e with a 2^-e <= 448 for the row's amax a (a = m 2^x, m in [0.5, 1): x - 9 when
// m <= 0.875, else x - 8), 0 for a = 0, clamped to +-64.  A denormal a has x <= -126: the clamp decides.
__device__ __forceinline__ int fp8_row_exponent(float amax) {
    const uint32_t bits = __float_as_uint(amax);
    if (bits == 0) return 0;
    const int field = (int)(bits >> 23);
    if (field == 0) return -kFp8ExpClamp;
    const int e = field - 126 - ((bits & 0x7fffffu) <= 0x600000u ? 9 : 8);
    return e < -kFp8ExpClamp ? -kFp8ExpClamp : (e > kFp8ExpClamp ? kFp8ExpClamp : e);
}

// 8 values times 2^-e (exact), clamped to +-448 (a no-op unless e hit its clamp), to 8 e4m3fn bytes, RNE
__device__ __forceinline__ u32x2_t fp8_rows_encode(const float (&d)[8], float inv_scale) {
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = fmaxf(-448.f, fminf(448.f, d[i] * inv_scale));
    u32x2_t r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int v = __builtin_amdgcn_cvt_pk_fp8_f32(a[4 * h], a[4 * h + 1], 0, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(a[4 * h + 2], a[4 * h + 3], v, true);
        r[h] = (uint32_t)v;
    }
    return r;
}

// the 8 e4m3fn bytes of q as fp32, in byte order (exact)
__device__ __forceinline__ void fp8_rows_decode(u32x2_t q, float (&f)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[h], false);
        const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[h], true);
        f[4 * h + 0] = lo[0];
        f[4 * h + 1] = lo[1];
        f[4 * h + 2] = hi[0];
        f[4 * h + 3] = hi[1];
    }
}

// 8 consecutive features of a KV-cache row: bf16(float(q) * scale).  The product is exact (3 mantissa bits times a power of
// two, no underflow at |e| <= 64) and so is the conversion: the 8 significant bits of bf16 hold it.
__device__ __forceinline__ bf16x8_t fp8_rows_value(u32x2_t q, float scale) {
    float f[8];
    fp8_rows_decode(q, f);
    bf16x8_t w;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (__bf16)(f[i] * scale);
    return w;
}
