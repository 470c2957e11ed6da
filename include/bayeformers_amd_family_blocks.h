/* bayeformers_amd_family_blocks.h — the decoder-block entries of the Gemma 1 / 2 / 3 and Qwen3 families.  Included by
 * bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as FAMILY_BLOCK_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_FAMILY_BLOCKS_H
#define BAYEFORMERS_AMD_FAMILY_BLOCKS_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The siblings of bf_add_rmsnorm / bf_rope_qk / bf_swiglu (bayeformers_amd.h: "the decoder layer's own ops") for decoder
 * layers those three do not cover: Gemma's (1 + weight) norms and its sandwich of four norms around the two residual adds
 * (Gemma 2 / 3), per-head q / k norms in front of the rotary embedding (Qwen3, Gemma 3), head size 256, and the tanh-GELU
 * gate.  The same manner: one launch each, 16-byte loads and stores, fp32 arithmetic in registers, one rounding into
 * `dtype` (BF16 | F16 | F32) where the text below names no other; no allocation, no synchronisation (capturable).
 * Unsupported arguments return 1 with bf_last_error() set; rows == 0 (an empty batch) returns 0 and launches nothing.
 *
 * bf_norm_add_rmsnorm — norm, residual add, norm in one pass over a row that stays in registers.  With round_T the
 * rounding into `dtype` and w(g) = weight_offset + g:
 *     u = d_gamma_pre ? round_T(x * rsqrt(mean(x^2) + eps_pre) * w(gamma_pre)) : x
 *     z = d_residual  ? round_T(residual + u) : u                                       -> d_sum_out (nullable)
 *     y = round_T(z * rsqrt(mean(z^2) + eps_out) * w(gamma_out))                        -> d_out
 * over the last axis; the statistics of y are taken from the rounded z.  (u is evaluated in fp64 and rounded once, so
 * that the add sees the correctly rounded norm.)  The two inner roundings are where HF's Gemma
 * modules round (the norm's `type_as(x)` and the add), so z is the tensor the unfused layer's next norm reads; without
 * d_gamma_pre it is bitwise the framework's `residual + x`.  weight_offset is 1 for Gemma's `(1 + weight)` norms and 0
 * for Llama's.  x, residual, z, y: [rows, N] of `dtype`, rows back to back; gamma_pre / gamma_out [N] of `param_dtype`
 * (BF_DT_F32 or `dtype`).  d_sum_out / d_out may be d_x or d_residual themselves (in place), no other overlap.
 * N % 8 == 0, N <= 8192, 16-byte aligned pointers. */
int bf_norm_add_rmsnorm(const void* d_x, const void* d_gamma_pre, const void* d_residual, const void* d_gamma_out,
                        int param_dtype, int weight_offset, void* d_sum_out, void* d_out, int dtype, int64_t rows, int N,
                        float eps_pre, float eps_out, void* stream);

/* bf_qknorm_rope — bf_rope_qk (its arguments, its bf_rope_t, its layouts and its in-place rule) at head_dim 64, 128 or
 * 256, with an optional RMSNorm over each head's head_dim elements in front of the rotation:
 *     n = x * rsqrt(mean_D(x^2) + eps) * (weight_offset + gamma),   out = n * cos + rotate_half(n) * sin
 * with gamma = d_gamma_q [head_dim] for the heads of q and d_gamma_k for those of k, of `param_dtype` (BF_DT_F32 or
 * `dtype`); n stays in fp32, the one rounding is the output's.  A NULL gamma leaves that tensor's heads as they are
 * (n = x): with both NULL this is bf_rope_qk's function, and at head_dim 64 and 128 bitwise its result.  weight_offset is
 * 0 (Qwen3) or 1 (Gemma 3). */
int bf_qknorm_rope(const void* d_q, const void* d_k, const void* d_cos, const void* d_sin, int cs_dtype,
                   const void* d_gamma_q, const void* d_gamma_k, int param_dtype, int weight_offset, float eps,
                   void* d_q_out, void* d_k_out, int dtype, const bf_rope_t* shape, void* stream);

/* bf_geglu — bf_swiglu's arguments and layouts with the tanh-GELU gate of the Gemma MLPs
 * (`gelu(gate_proj(x), approximate="tanh") * up_proj(x)`):
 *     y = gate / (1 + exp(-2 k)) * up,   k = sqrt(2 / pi) * (gate + 0.044715 gate^3)
 * which is 0.5 gate (1 + tanh k) up written so that nothing cancels for negative gates; evaluated through exp(-|2k|), so
 * that nothing overflows either.  Finite for every finite input whose result is (gate -> -inf gives -0 * up, gate -> +inf
 * gate * up). */
int bf_geglu(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, void* d_out,
             int64_t out_row_stride, int dtype, int64_t rows, int N, void* stream);

#ifdef __cplusplus
}
#endif

#include "bayeformers_amd_family_blocks_bwd.h" /* the backward of the three: a header and a ctypes table of their own */

#endif /* BAYEFORMERS_AMD_FAMILY_BLOCKS_H */
