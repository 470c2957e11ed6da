/* bayeformers_amd_fp8.h — the FP8 kept-weight entries of the C-ABI (Model.pinned_samples(keep_weights="fp8")).  Included
 * by bayeformers_amd.h (include that one): the same conventions, the same library, the same BF_VERSION; bound by
 * bayeformers_amd/_C.py as FP8_SYMBOLS.  Additions only: nothing bayeformers_amd.h declares changed with them.
 */
#ifndef BAYEFORMERS_AMD_FP8_H
#define BAYEFORMERS_AMD_FP8_H

#include "bayeformers_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- centred FP8 rows: the format ---------------------------------------------------------------------------------
 * The S weight draws of a layer differ from their posterior mean by about sigma; rounding the draws themselves to 8 bits
 * would add noise of the posterior's own size.  So one 16-bit copy of the mean is kept for all samples and only each
 * draw's DEVIATION from it is stored in 8 bits.  For sampled weights W16 [S][N][K] (bf16) and the centre
 * C16 = bf16_rne(mu) [N][K]:
 *   d            = float(W16) - float(C16)                                   (fp32 subtraction)
 *   a            = max_k |d|                                                 per row (s, n)
 *   e            = the smallest integer with a * 2^-e <= 448: with a = m * 2^x, m in [0.5, 1), e = x - 9 if m <= 0.875,
 *                  else x - 8; e = 0 if a = 0; e is clamped to [-64, 64]
 *   scale[s][n]  = 2^e                                                       fp32
 *   q[s][n][k]   = e4m3fn_rne(clamp(d * 2^-e, -448, 448))                    one byte, OCP E4M3 (finite-only, bias 7)
 * The clamp only acts when e hit its bound: otherwise |d * 2^-e| <= 448 already, so no conversion relies on a saturation
 * mode.  The dequantised weight is
 *   W^[s][n][k]  = bf16_rne(fp32(float(q) * scale + float(C16)))
 * where the product is exact (a power of two, no underflow for |e| <= 64): one fp32 rounding, then one bf16 rounding.
 * The error W^ - W16 is at most 2^-4 |d| (the e4m3 step) plus one bf16 rounding of W^.  Only bf16 is taken: fp16 lacks
 * the exponent range that makes W^ well defined for every scale, and fp32 weights are not kept in this form.
 * All entries are asynchronous on `stream`, allocate nothing and never synchronise (capturable); they return 0, or 1
 * with bf_last_error() set, before any launch. */

/* q, scale <- W16, C16.  d_w [S][N][K] bf16 (w_dtype must be BF_DT_BF16), d_center [N][K] bf16, d_q [S][N][K] bytes,
 * d_scale [S][N] fp32.  One workgroup per row.  Rows are read with 16-byte loads when K % 8 == 0 and d_w / d_center are
 * 16-byte, d_q 8-byte aligned; any other K or alignment runs element by element.  S * N < 2^31. */
int bf_fp8_rows_quantize(const void* d_w, int w_dtype, const void* d_center, void* d_q, float* d_scale, int S, int N, int K,
                         void* stream);
/* W^ [S][N][K] bf16 <- q, scale, C16 (w_dtype must be BF_DT_BF16). */
int bf_fp8_rows_dequantize(const void* d_q, const float* d_scale, const void* d_center, void* d_w_out, int w_dtype, int S,
                           int N, int K, void* stream);

/* y[s] = act(x[s] W^_s^T + bias[s]) on the quantised rows: bf_gemm_nt_skinny's shapes (bf16 x [S][M][K] with x sample
 * stride >= M*K elements, bf16 y [S][M][N], 1 <= M <= bf_gemm_nt_skinny_max_rows(), K % 32 == 0, any N, S <= 65535; bias
 * [S][N] fp32 or NULL; act BF_ACT_NONE / BF_ACT_GELU) and its structure: the weights are streamed once, one byte each
 * (the centre is read again per sample and is meant to come from cache), W^ is formed in registers — bitwise what
 * bf_fp8_rows_dequantize writes — and multiplied by v_mfma_f32_16x16x32_bf16 with fp32 accumulation; K is split over
 * workgroups by bf_gemm_nt_skinny's rule with a second launch that sums the fp32 partials in split order.  No atomics:
 * bitwise reproducible.  d_workspace holds bf_gemm_nt_skinny_fp8_workspace_bytes(S, M, N, K) bytes (NULL when that is 0),
 * 16-byte aligned.  Refused: x / y not bf16, a shape outside the above, x / q / center or the sample stride not 16-byte
 * aligned, y not 8-byte aligned, a workspace that is missing or too small. */
int bf_gemm_nt_skinny_fp8(const void* d_x, int x_dtype, int64_t x_sample_stride, const void* d_q, const float* d_scale,
                          const void* d_center, const float* d_bias /* nullable */, void* d_y, int y_dtype, int S, int M,
                          int N, int K, int act, void* d_workspace, size_t workspace_bytes, void* stream);
size_t bf_gemm_nt_skinny_fp8_workspace_bytes(int S, int M, int N, int K);

#ifdef __cplusplus
}
#endif
#endif /* BAYEFORMERS_AMD_FP8_H */
