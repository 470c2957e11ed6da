/* bayeformers_amd_family_blocks_bwd.h — the backward of the decoder-block entries of the Gemma 1 / 2 / 3 and Qwen3 families
 * (bayeformers_amd_family_blocks.h, which includes this header: include bayeformers_amd.h).  The same conventions, the same
 * library, the same BF_VERSION; bound by bayeformers_amd/_C.py as FAMILY_BLOCK_BWD_SYMBOLS, which this header matches entry
 * for entry as bayeformers_amd_family_blocks.h matches FAMILY_BLOCK_SYMBOLS.  Additions only.
 */
#ifndef BAYEFORMERS_AMD_FAMILY_BLOCKS_BWD_H
#define BAYEFORMERS_AMD_FAMILY_BLOCKS_BWD_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The manner of bf_add_rmsnorm_bwd / bf_rope_qk_bwd / bf_swiglu_bwd: fp32 arithmetic on 16-byte loads, one rounding into
 * `dtype`, no allocation, no synchronisation (capturable), no float atomics — parameter gradients are fp32, reduced in a
 * fixed order through a caller-provided workspace, and bitwise repeatable.
 *
 * bf_norm_add_rmsnorm_bwd — the gradients of bf_norm_add_rmsnorm from z (its d_sum_out, or x itself when neither a gamma_pre
 * nor a residual changed it) and, with d_gamma_pre, its input x.  With w(g) = weight_offset + g and
 * r(v) = rsqrt(mean(v^2) + eps):
 *     a = w(gamma_out) o dy,   dz = r(z) a - z r(z)^3 mean(z o a) + dz_in,       dgamma_out = sum_rows dy o z r(z)
 *     b = w(gamma_pre) o dz,   dx = r(x) b - x r(x)^3 mean(x o b),               dgamma_pre = sum_rows dz o x r(x)
 * dz is the gradient of the residual (and of x without d_gamma_pre: d_dx is then not written); stage 1 takes dz unrounded,
 * in fp32.  d_dz_in (nullable): the gradient that reached z through its other consumer.  d_dy may be NULL when only the
 * sum was consumed (d_dz_in is then required): dz = dz_in, dgamma_out = 0.  With d_gamma_pre d_dz may be NULL (no
 * residual: nobody reads dz).  d_dz may be d_dy or d_dz_in themselves and d_dx may be d_dz; no other overlap.
 * d_dgamma_pre / d_dgamma_out: [N] fp32.  Both sums of squares are taken in fp64 and each dgamma term is formed in fp64.
 * Two launches: the row pass and one reduction of the workgroups' partial rows.  rows == 0 zeroes the dgammas.
 * N % 8 == 0, N <= 8192. */
size_t bf_norm_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int N, int has_gamma_pre);
int bf_norm_add_rmsnorm_bwd(const void* d_x, const void* d_z, const void* d_gamma_pre, const void* d_gamma_out, int param_dtype,
                            int weight_offset, const void* d_dy, const void* d_dz_in, void* d_dz, void* d_dx,
                            float* d_dgamma_pre, float* d_dgamma_out, void* d_workspace, size_t workspace_bytes, int dtype,
                            int64_t rows, int N, float eps_pre, float eps_out, void* stream);

/* bf_qknorm_rope_bwd — the transpose of bf_qknorm_rope.  d_dq_out [B, H, T, D] / d_dk_out [B, Hkv, T, D]: the gradients of
 * its outputs, read through shape->q_stride / k_stride (any layout the forward takes); shape->q_out_stride / k_out_stride
 * are not read: d_dq / d_dk are written laid out [B, T, heads, D], back to back, and d_q / d_k — the forward's inputs,
 * needed (and read) only for a tensor that has a gamma — are read in that layout.  With do the incoming gradient:
 *     dn1 = do1 c1 + do2 s2,   dn2 = do2 c2 - do1 s1                      (the transpose for unequal table halves as well)
 *     b = (weight_offset + gamma) o dn,   dx = r b - x r^3 mean_D(x o b),   dgamma = sum_{b, t, heads} dn o x r
 * with r = rsqrt(mean_D(x^2) + eps) recomputed; a tensor whose gamma is NULL is only rotated (dx = dn) and its dgamma is
 * not written.  d_dgamma_q / d_dgamma_k: [head_dim] fp32.  The workspace is needed only with a gamma. */
size_t bf_qknorm_rope_bwd_workspace_bytes(const bf_rope_t* shape, int has_gamma);
int bf_qknorm_rope_bwd(const void* d_dq_out, const void* d_dk_out, const void* d_q, const void* d_k, const void* d_cos,
                       const void* d_sin, int cs_dtype, const void* d_gamma_q, const void* d_gamma_k, int param_dtype,
                       int weight_offset, float eps, void* d_dq, void* d_dk, float* d_dgamma_q, float* d_dgamma_k,
                       void* d_workspace, size_t workspace_bytes, int dtype, const bf_rope_t* shape, void* stream);

/* bf_geglu_bwd — bf_swiglu_bwd's arguments and layouts (the two gradients may be the halves of one [rows, 2N] buffer) for
 * bf_geglu: with 2k = g (2c + 2c 0.044715 g^2), c = sqrt(2 / pi), s = sigmoid(2k):
 *     dup = dy g s,   dgate = dy u s (1 + g (1 - s) 2c (1 + 3 * 0.044715 g^2)).
 * Finite wherever the mathematical result is: g -> +inf gives (dy u, dy g), g -> -inf gives (0, 0) (signed zeros). */
int bf_geglu_bwd(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, const void* d_dy,
                 int64_t dy_row_stride, void* d_dgate, int64_t dgate_row_stride, void* d_dup, int64_t dup_row_stride, int dtype,
                 int64_t rows, int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_FAMILY_BLOCKS_BWD_H */
