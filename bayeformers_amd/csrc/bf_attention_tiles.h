// bf_attention_tiles.h — MFMA fragment layouts and LDS images shared by the attention kernels of bf_attention.hip,
// bf_attention_bwd.hip, bf_attention_gqa.hip and bf_attention_decode.hip (bf16 / fp16 operands, mfma_f32_16x16x32, head
// size 64, 128 or 256).  The contract all of them lean on:
//   * lane (li, lg) = (lane & 15, lane >> 4).  As an operand it holds 8 consecutive features (k group lg) of row / column li.
//     S^T = K Q^T with the keys as rows leaves it 4 consecutive keys, blk*16 + 4 lg + 0..3, of ONE query li per 16-key block:
//     a query's softmax statistics are in-lane values + two cross-lane steps (the dk/dv kernels swap the roles);
//   * two neighbouring blocks are then the 8-element column operand of the next product as they stand (pack2), its k index
//     a fixed permutation of the keys: (2c)*16 + 4 lg + 0..3, then (2c + 1)*16 + 4 lg + 0..3.  tr_frag(c) applies the same
//     order to the other operand, straight out of a row-major image through gfx950's LDS transpose read (ds_read_b64_tr_b16);
//   * the dropout keep-bit layout (AttnParams, bf_attention.hip: bit c*8 + e*4 + j of word lg) is that order written
//     down, and the backward kernels read the bits by it.  Changing the order changes all of these at once.
#pragma once
#include "bf_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// tanh for the soft-capped logits (gfx950 has no tanh instruction): 1 - 2 / (1 + e^2x) from the exp2 and rcp units.  e^2x
// overflows to +inf (rcp gives 0: th = 1) and underflows to 0 (th = -1): saturation, never NaN, at both ends.  Near 0 that
// form cancels — its error is an ulp of 1, which is all of a tiny x — so the result is held between x and x - x^3 / 3, which
// bracket tanh(x) for either sign (one median instruction, no branch): the error is the smaller of the two, and a cap far
// above the logits gives the uncapped scores to rounding.  (An overflowing x^3 leaves -inf / +inf as the far bound.)
__device__ __forceinline__ float softcap_tanh(float x) {
    const float e = __builtin_amdgcn_exp2f(x * (2.0f * LOG2E));
    const float th = fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
    return __builtin_amdgcn_fmed3f(th, x, fmaf(x * x * x, -1.0f / 3.0f, x));
}

typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;

template <typename T>
struct Mfma;
template <>
struct Mfma<__bf16> {
    using frag = bf16x8_t;
    using half4 = bf16x4_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mfma<_Float16> {
    using frag = f16x8_t;
    using half4 = f16x4_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

// Row stride of the LDS images: swizzled (16-byte chunk ^= row & 7, for direct row-operand reads) and padded (+32 B, for
// the transpose reads: the 8 rows a 32-lane half of one touches tile one bank row)
template <int HD>
struct Rows {
    static constexpr int SWZ = HD * 2;
    static constexpr int PAD = HD * 2 + 32;
};

// Key tile and workgroups per CU of the causal forward kernels, per head size: bf_attention_gqa.hip's forward (its Shape gives
// the reasons) and bf_attention_chunk.hip's, whose rows are bitwise that forward's only while both walk the same key tiles.
template <int HD>
struct FwdShape;
template <>
struct FwdShape<64> {
    static constexpr int KT = 128, MINB = 3;
};
template <>
struct FwdShape<128> {
    static constexpr int KT = 128, MINB = 2;
};
template <>
struct FwdShape<256> {
    static constexpr int KT = 64, MINB = 1;
};

// stage rows row0 .. row0 + NR - 1 of a [tokens][stride] tensor into the swizzled and / or the padded image
template <typename T, int HD, int NR, int NT>
__device__ __forceinline__ void stage(const T* base, long long stride, int row0, char* swz, char* pad, int tid) {
    constexpr int CPR = HD / 8;  // 16-byte chunks per row
    static_assert((NR * CPR) % NT == 0, "whole passes");
#pragma unroll
    for (int i = 0; i < NR * CPR / NT; ++i) {
        const int c = tid + NT * i, row = c / CPR, c8 = c % CPR;
        const f32x4_t x = *reinterpret_cast<const f32x4_t*>(base + (long long)(row0 + row) * stride + c8 * 8);
        if (swz) *reinterpret_cast<f32x4_t*>(swz + row * Rows<HD>::SWZ + ((c8 ^ (row & 7)) << 4)) = x;
        if (pad) *reinterpret_cast<f32x4_t*>(pad + row * Rows<HD>::PAD + (c8 << 4)) = x;
    }
}

// ... of a tensor that ends at row `last`: a row past it re-reads row `last` (a finite value of the caller's, never what lies
// behind the tensor; no branch).  The caller gives such rows no weight and stores nothing for them.
template <typename T, int HD, int NR, int NT>
__device__ __forceinline__ void stage_clamped(const T* base, long long stride, int row0, int last, char* swz, char* pad,
                                              int tid) {
    constexpr int CPR = HD / 8;
    static_assert((NR * CPR) % NT == 0, "whole passes");
#pragma unroll
    for (int i = 0; i < NR * CPR / NT; ++i) {
        const int c = tid + NT * i, row = c / CPR, c8 = c % CPR;
        const f32x4_t x = *reinterpret_cast<const f32x4_t*>(base + (long long)min(row0 + row, last) * stride + c8 * 8);
        if (swz) *reinterpret_cast<f32x4_t*>(swz + row * Rows<HD>::SWZ + ((c8 ^ (row & 7)) << 4)) = x;
        if (pad) *reinterpret_cast<f32x4_t*>(pad + row * Rows<HD>::PAD + (c8 << 4)) = x;
    }
}

// row-operand fragment (16 rows x 32 features, half dh) of block `blk` of a swizzled image: lane (row li, k group lg)
template <typename T, int HD>
__device__ __forceinline__ typename Mfma<T>::frag row_frag(const char* swz, int blk, int dh, int li, int lg) {
    const int row = blk * 16 + li;
    return *reinterpret_cast<const typename Mfma<T>::frag*>(swz + row * Rows<HD>::SWZ + (((dh * 4 + lg) ^ (row & 7)) << 4));
}

// transposed fragment of a row-major image with rows of ROW bytes: rows = features db*16 + li, k = the 32 image rows
// {(2c)*16 + 4 lg + 0..3, (2c+1)*16 + 4 lg + 0..3}, by two LDS transpose reads (the 16 lanes of a group point at a
// [4 rows][16 features] block: lane -> row li >> 2, features 4 * (li & 3) .., each gets its column = 4 rows of feature li)
template <typename T, int ROW>
__device__ __forceinline__ typename Mfma<T>::frag tr_frag_row(const char* pad, int c, int db, int li, int lg) {
    const char* blk = pad + (lg * 4 + (li >> 2)) * ROW + (db * 16 + (li & 3) * 4) * 2;
    const s16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(blk + (2 * c) * 16 * ROW));
    const s16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(blk + (2 * c + 1) * 16 * ROW));
    const s16x8_t ab = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(typename Mfma<T>::frag, ab);
}

// ... of a padded image of head size HD
template <typename T, int HD>
__device__ __forceinline__ typename Mfma<T>::frag tr_frag(const char* pad, int c, int db, int li, int lg) {
    return tr_frag_row<T, Rows<HD>::PAD>(pad, c, db, li, lg);
}

template <typename T>
__device__ __forceinline__ typename Mfma<T>::frag pack2(const f32x4_t a, const f32x4_t b) {
    const f32x8_t v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_convertvector(v, typename Mfma<T>::frag);
}

}  // namespace
