// bf_vec8.h — 16-byte row I/O of the streaming kernels (bf_norm.hip, bf_decoder_blocks.hip): 8 consecutive elements of
// bf16 / fp16 / fp32 <-> 8 floats in registers.
#pragma once
#include "bf_common.h"

// 8 consecutive elements <-> 8 floats
__device__ __forceinline__ void load8(const __bf16* p, float (&v)[8]) {
    const bf16x8_t t = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}
__device__ __forceinline__ void load8(const _Float16* p, float (&v)[8]) {
    const f16x8_t t = *reinterpret_cast<const f16x8_t*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = a[i], v[4 + i] = b[i];
}
// The normalised rows are written through (sc0 sc1).  Measured on the whole BERT-base step, three interleaved rounds on one
// box (profiles/r3k_layernorm_store_policy.txt): nontemporal 8.81-8.87 ms, plain 8.78-8.79, sc1 8.71-8.77, sc0 sc1 8.70-8.75:
// write-through rows are what the GEMM that reads them next (cold, from another XCD's point of view) finds fastest.
__device__ __forceinline__ void st16(f32x4_t* p, f32x4_t v) {
    // (inline asm: there is no builtin for a flat-addressed store with these cache bits.  The trailing s_nop keeps the
    // compiler's next instruction from overwriting the data registers before the store has read them — it does not pad
    // hazards of instructions inside an asm statement)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store8(__bf16* p, const float (&v)[8]) {
    const bf16x8_t t = __builtin_convertvector((f32x8_t{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}), bf16x8_t);
    st16(reinterpret_cast<f32x4_t*>(p), __builtin_bit_cast(f32x4_t, t));
}
__device__ __forceinline__ void store8(_Float16* p, const float (&v)[8]) {
    const f16x8_t t = __builtin_convertvector((f32x8_t{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}), f16x8_t);
    st16(reinterpret_cast<f32x4_t*>(p), __builtin_bit_cast(f32x4_t, t));
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    st16(reinterpret_cast<f32x4_t*>(p), f32x4_t{v[0], v[1], v[2], v[3]});
    st16(reinterpret_cast<f32x4_t*>(p + 4), f32x4_t{v[4], v[5], v[6], v[7]});
}
